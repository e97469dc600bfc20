"""Round schedule of the lane-parallel 6x6 Jacobi SVD (jacobi_svd6_lanes, csrc/svo_device.hpp).

The reference sweeps the row pairs in cyclic order, (0,1) (0,2) .. (0,5) (1,2) .. (4,5), sweep after
sweep. A pair reads and writes only its two rows, so a pair can run once the last earlier pair on
each of its rows has run. Scheduled as early as possible, the stream settles into a body of 6 rounds
per sweep; this module derives that body and prints it as the C tables of the header.

    python3 tools/svd_schedule.py        # the two constexpr lines of svo_device.hpp
"""
N = 6
PAIRS = [(i, j) for i in range(N - 1) for j in range(i + 1, N)]
MAX_SWEEPS = 30


def asap(n_sweeps):
    """{round: [(sweep, i, j), ...]} of the first n_sweeps sweeps, each pair as early as its rows allow."""
    last = [0] * N
    rounds = {}
    for s in range(n_sweeps):
        for i, j in PAIRS:
            rd = max(last[i], last[j]) + 1
            last[i] = last[j] = rd
            rounds.setdefault(rd, []).append((s, i, j))
    return rounds


def body():
    """The steady-state 6-round body: [[(lag, i, j), ...] per position], lag 1 = pair of sweep t - 1
    in body iteration t. Taken from a sweep in the middle of a long stream and checked periodic."""
    rounds = asap(8)
    per = None
    for start in (6 * 3 + 1, 6 * 4 + 1):    # rounds of iterations 3 and 4 (0-based sweeps 3 and 4 start)
        t = (start - 1) // 6
        b = [sorted((t - s, i, j) for s, i, j in rounds[start + q]) for q in range(6)]
        assert per is None or b == per, "ASAP schedule not periodic"
        per = b
    return per


def tables(b=None):
    """(partner, lag) words per position: nibble r of partner = row paired with r (r itself when idle,
    rows 6 and 7 always idle); bit r of lag = row r's pair belongs to sweep t - 1."""
    b = body() if b is None else b
    partner, lagw = [], []
    for pos in b:
        p = list(range(8))
        lw = 0
        for lag, i, j in pos:
            p[i], p[j] = j, i
            if lag:
                lw |= (1 << i) | (1 << j)
        partner.append(sum(x << (4 * r) for r, x in enumerate(p)))
        lagw.append(lw)
    return partner, lagw


def run(n_sweeps_before_stop=None, b=None):
    """Executes the body like jacobi_svd6_lanes does. Returns (order, stops): order = list of rounds,
    each a list of (sweep, i, j) that run; stops = {t: set of pairs of sweep t - 1 that had run and
    list of sweep t pairs that had run} at every stop check (after position 3 of iteration t >= 1).
    With n_sweeps_before_stop = S the loop stops at the check of iteration S (sweep S - 1 rotated
    nothing); None runs to the cap."""
    b = body() if b is None else b
    order, stops = [], {}
    t = 0
    while True:
        for q in range(6):
            rd = [(t - lag, i, j) for lag, i, j in b[q] if 0 <= t - lag < MAX_SWEEPS]
            order.append(rd)
            if q == 2:
                if t >= 1:
                    done = [x for r in order for x in r]
                    stops[t] = done
                if t == MAX_SWEEPS or (n_sweeps_before_stop is not None and t == n_sweeps_before_stop):
                    return order, stops, t
        t += 1


def c_lines():
    partner, lagw = tables()
    return ("constexpr uint32_t kSvdPartner[6] = {%s};\n" % ", ".join("0x%08Xu" % x for x in partner) +
            "constexpr uint32_t kSvdLag[6] = {%s};" % ", ".join("0x%02Xu" % x for x in lagw))


if __name__ == "__main__":
    for q, pos in enumerate(body()):
        print("// pos %d: %s" % (q + 1, " ".join("(%d,%d)%s" % (i, j, " t-1" if lag else "") for lag, i, j in pos)))
    print(c_lines())
