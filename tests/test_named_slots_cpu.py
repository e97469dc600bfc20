"""The ctx's view of the slots a call names (csrc/svo_named_slots.hpp) in a stand-alone program
(tests/cpp/named_slots_check.cpp) built with g++, once plain and once with the address and undefined-behaviour
sanitizers: the first bad position, and the split over groups. The asserts are in the program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the program, plain and sanitized: {name: path}"""
    d = tmp_path_factory.mktemp("named_slots")
    gxx = shutil.which("g++")
    assert gxx
    src = os.path.join(ROOT, "tests", "cpp", "named_slots_check.cpp")
    common = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", src]
    out = {"plain": str(d / "named_slots_check"), "sanitized": str(d / "named_slots_check_san")}
    subprocess.check_call(common + ["-o", out["plain"]])
    subprocess.check_call(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-o", out["sanitized"]])
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_named_slots(built, which):
    r = subprocess.run([built[which]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "named slots ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
