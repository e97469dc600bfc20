"""The voxel maps of include/svo_hip.h ("voxel maps") as plain numpy, written from that section alone: the key and
sub-voxel offsets of a record in float32, the fusion in integers modulo 2^32, the extraction in float64 and 64-bit
integers. Two statements: a vectorised one whose result cannot depend on the order of its input (np.unique and sums
modulo 2^32), and beside it a scalar one that keeps a dict and visits record after record. A map is here the sorted
keys and their eight accumulators; where an entry lies in the table is no part of the statement (home() is the
diagnostic fact the cases craft probe chains with)."""
import numpy as np

F = np.float32
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("color", "u1", (3,)), ("flags", "u1")])
DROPPED = 0x80
IGNORE_DURING_REFINEMENT, IGNORE_COMPLETELY, IGNORE_TEMPORARY = 1, 2, 4
EMPTY = 2**64 - 1
HASH = 0x9E3779B97F4A7C15
BIAS = 1048576                         # 2^20
MASK32 = np.uint64(0xFFFFFFFF)


def map_bytes(log2_capacity):
    return 256 + (40 << log2_capacity)


def load_limit(log2_capacity):
    cap = 1 << log2_capacity
    return cap - cap // 4


def home(key, log2_capacity):
    return ((int(key) * HASH) & EMPTY) >> (64 - log2_capacity)


def key_parts(key):
    key = int(key)
    return key >> 42, (key >> 21) & 0x1FFFFF, key & 0x1FFFFF


def records(xyz, color=(0, 0, 0), flags=0):
    """POINT records of an [n, 3] array of coordinates"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    r = np.zeros(len(xyz), POINT)
    r["x"], r["y"], r["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r["color"] = np.asarray(color, np.uint8)
    r["flags"] = flags
    return r


# ------------------------------------------------------------------------------------------------ vectorised

def classify(rec, voxel, drop_flags):
    """of every record: offered, inside (of the offered), key (uint64), offsets uint64 [n, 3]"""
    voxel = F(voxel)
    offered = (rec["flags"] & (DROPPED | drop_flags)) == 0
    inside = offered.copy()
    key = np.zeros(len(rec), np.uint64)
    offs = np.zeros((len(rec), 3), np.uint64)
    with np.errstate(all="ignore"):
        for j, c in enumerate("xyz"):
            t = (rec[c].astype(F) / voxel).astype(F)
            q = np.floor(t).astype(F)
            ok = np.abs(q) < F(1048576.0)                           # False for a NaN
            inside &= ok
            qi = np.where(ok, q, F(0)).astype(np.int64) + BIAS
            frac = ((t - q).astype(F) * F(256.0)).astype(F)
            o = np.minimum(255, np.where(ok, frac, F(0)).astype(np.uint32)).astype(np.uint64)
            key = (key << np.uint64(21)) | qi.astype(np.uint64)
            offs[:, j] = o
    return offered, inside, key, offs


class Map:
    """voxel, log2_capacity, drop_flags; keys (sorted uint64) and acc uint64 [n, 8] (count, sx, sy, sz, sr, sg, sb,
    last; each < 2^32); the counters of svo_voxel_map_info"""

    def __init__(self, voxel, log2_capacity, drop_flags=0):
        self.voxel, self.log2_capacity, self.drop_flags = F(voxel), int(log2_capacity), int(drop_flags)
        self.keys = np.zeros(0, np.uint64)
        self.acc = np.zeros((0, 8), np.uint64)
        self.n_fused = self.n_outside = 0

    @property
    def n_voxels(self):
        return len(self.keys)

    def admits(self, n_records):
        """the load bound"""
        return self.n_voxels + n_records <= load_limit(self.log2_capacity)

    def fuse(self, rec, stamp):
        offered, inside, key, offs = classify(rec, self.voxel, self.drop_flags)
        self.n_outside += int((offered & ~inside).sum())
        self.n_fused += int(inside.sum())
        k = key[inside]
        rows = np.concatenate([np.ones((len(k), 1), np.uint64), offs[inside], rec["color"][inside].astype(np.uint64)], axis=1)
        all_keys = np.concatenate([self.keys, k])
        uniq, inv = np.unique(all_keys, return_inverse=True)
        sums = np.zeros((len(uniq), 7), np.uint64)
        np.add.at(sums, inv, np.concatenate([self.acc[:, :7], rows]))
        last = np.zeros(len(uniq), np.uint64)
        np.maximum.at(last, inv, np.concatenate([self.acc[:, 7], np.full(len(k), stamp, np.uint64)]))
        self.keys, self.acc = uniq, np.concatenate([sums & MASK32, last[:, None]], axis=1)

    def extract(self, min_count=0, min_stamp=0):
        keep = (self.acc[:, 0] >= max(1, min_count)) & (self.acc[:, 7] >= min_stamp)
        keys, acc = self.keys[keep], self.acc[keep]
        out = np.zeros(len(keys), POINT)
        count = acc[:, 0]
        for j, c in enumerate("xyz"):
            cell = ((keys >> np.uint64(21 * (2 - j))) & np.uint64(0x1FFFFF)).astype(np.int64) - BIAS
            mean = acc[:, 1 + j].astype(np.float64) / count.astype(np.float64)
            out[c] = (((cell.astype(np.float64) + (mean + 0.5) / 256.0) * np.float64(self.voxel))).astype(F)
            out["color"][:, j] = np.minimum(255, (acc[:, 4 + j] + count // np.uint64(2)) // count).astype(np.uint8)
        return out


# ------------------------------------------------------------------------------------------------ scalar

def scalar_key(x, y, z, voxel):
    """(key, (ox, oy, oz)) of one point, or None: outside"""
    voxel = F(voxel)
    key, offs = 0, []
    with np.errstate(all="ignore"):
        for c in (F(x), F(y), F(z)):
            t = F(c / voxel)
            q = F(np.floor(t))
            if not abs(q) < F(1048576.0):
                return None
            key = key << 21 | (int(q) + BIAS)
            offs.append(min(255, int(F(F(t - q) * F(256.0)))))
    return key, tuple(offs)


class ScalarMap:
    def __init__(self, voxel, log2_capacity, drop_flags=0):
        self.voxel, self.log2_capacity, self.drop_flags = F(voxel), int(log2_capacity), int(drop_flags)
        self.entries = {}
        self.n_fused = self.n_outside = 0

    @property
    def n_voxels(self):
        return len(self.entries)

    def fuse(self, rec, stamp):
        for r in rec:
            if int(r["flags"]) & (DROPPED | self.drop_flags):
                continue
            kp = scalar_key(r["x"], r["y"], r["z"], self.voxel)
            if kp is None:
                self.n_outside += 1
                continue
            e = self.entries.setdefault(kp[0], [0] * 8)
            for j, add in enumerate((1,) + kp[1] + tuple(int(c) for c in r["color"])):
                e[j] = (e[j] + add) & 0xFFFFFFFF
            e[7] = max(e[7], int(stamp))
            self.n_fused += 1

    def extract(self, min_count=0, min_stamp=0):
        out = []
        for key in sorted(self.entries):
            e = self.entries[key]
            if e[0] < max(1, min_count) or e[7] < min_stamp:
                continue
            p = np.zeros((), POINT)
            for j, (c, cell) in enumerate(zip("xyz", key_parts(key))):
                p[c] = F((float(cell - BIAS) + (e[1 + j] / e[0] + 0.5) / 256.0) * float(self.voxel))
                p["color"][j] = min(255, (e[4 + j] + e[0] // 2) // e[0])
            out.append(p)
        return np.array(out, POINT) if out else np.zeros(0, POINT)


def run(case, cls=Map):
    """the maps of a case (tests/voxel_cases.py) after all its calls; a call the load bound rejects changes nothing"""
    maps = [cls(*m) for m in case["maps"]]
    for call in case["calls"]:
        per_map = [sum(len(r) for r, m, _ in call if m == i) for i in range(len(maps))]
        if not all(Map.admits(mp, n) for mp, n in zip(maps, per_map)):
            continue
        for rec, m, stamp in call:
            maps[m].fuse(rec, stamp)
    return maps
