"""The launch-size switch of the N = 1024 / 256 passes, restated for the tests.

`hbx::pass_launch_small` (csrc/hbx_internal.hpp) picks, per launch, between the one-block-per-workgroup
forms of the bit path's first pass and of the column pass k_col2 and their walking forms.
`walking(n, planes, jobs, pair)` is its negation in Python: tests/test_gpu_launch_size.py asserts through
it which form each of its launches runs, and tests/test_launch_size_host.py holds it to the C++ function
(tests/c/launch_size_table.hip), so a change of the threshold cannot silently turn those GPU tests into
tests of one form only.
"""
SMALL_BLOCKS = 2048            # kSmallBlocks
ROW_NT = 256                   # row_nt(R): threads of a first-pass workgroup
LANE_GROUP = {1024: 32, 256: 16, 64: 8}          # N = R * R
ITERS = {32: 4, 16: 2, 8: 1}   # pass_rowfwd_iters = pass_col2_iters: row blocks / lines a workgroup walks
TABLE_R = (32, 16, 8)
TABLE_P = (2, 4, 8, 12, 24)


def _small(r: int, planes: int, jobs: int, pair: bool) -> bool:
    if r not in (32, 16):
        return False           # N = 64: one form of each kernel
    n = r * r
    row_blocks = n // (ROW_NT // r)                 # per plane pair
    rf_blocks = jobs * (1 if pair else planes // 2) * row_blocks // ITERS[r]
    col_blocks = jobs * (2 if pair else planes) * ((n // 2) // ((256 // r) * ITERS[r]))
    return rf_blocks < SMALL_BLOCKS and col_blocks < SMALL_BLOCKS


def walking(n: int, planes: int, jobs: int, pair: bool = False) -> bool:
    """Whether one launch of `jobs` jobs at N = n with `planes` planes per group (pair: the plane-cached
    step, one plane pair per job) runs the walking forms.  N = 896 has its own launcher and no switch."""
    if n not in LANE_GROUP:
        raise ValueError(f"N = {n}: no launch-size switch")
    return not _small(LANE_GROUP[n], int(planes), int(jobs), bool(pair))


def first_walking(n: int, planes: int, pair: bool = False, limit: int = 1 << 16):
    """The smallest job count of a launch that runs the walking forms (None: none up to limit)."""
    return next((j for j in range(1, limit + 1) if walking(n, planes, j, pair)), None)


def launches(total: int, per_launch: int):
    """Job counts of the launches that `total` jobs make in chunks of `per_launch`."""
    return [min(per_launch, total - i) for i in range(0, total, per_launch)]


def table():
    """The lines tests/c/launch_size_table.hip prints."""
    out = []
    for r in TABLE_R:
        for p in TABLE_P:
            for pair in (0, 1):
                first = first_walking(r * r, p, bool(pair))
                out.append(f"{r} {p} {pair} {'never' if first is None else first}")
    return out
