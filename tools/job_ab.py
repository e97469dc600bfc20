"""What the bench tools' --sgm legs share: queued job objects timed against each other in one process, the
legs alternating, and one result file that several tools write a key of."""
import json
import os
import statistics
import time

import torch


def alternate_jobs(device, jobs, repeats):
    """jobs: {name: job object}. Each leg is job.submit().wait() between two device synchronisations (wall clock); every
    job runs once untimed, then `repeats` rounds run the legs in turn. Returns {name: {"ms": median, "ms_all": [...]}}."""
    for job in jobs.values():
        job.submit().wait()
    all_ms = {name: [] for name in jobs}
    for _ in range(repeats):
        for name, job in jobs.items():
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            job.submit().wait()
            torch.cuda.synchronize(device)
            all_ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"ms": statistics.median(v), "ms_all": v} for name, v in all_ms.items()}


def ratios(timed, pairs):
    """{"a / b": median(a) / median(b)} for the named pairs of alternate_jobs' result"""
    return {f"{a} / {b}": timed[a]["ms"] / timed[b]["ms"] for a, b in pairs}


def sgm_dict(spec, lr):
    """--sgm P1,P2[,CAP] and a tolerance (0 or None: unchecked) as the sgm= of the Python layers"""
    p = [int(v) for v in spec.split(",")]
    return dict(p1=p[0], p2=p[1], cost_cap=p[2] if len(p) > 2 else 4095, lr_check=lr or None)


def merge_result(path, key, value):
    """the JSON object in `path` (made if missing) with `key` set to `value`"""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out
