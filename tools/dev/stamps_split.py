"""clocks per row of the full and of the other tiles of a cfg2 bundle launch, from a SA_HIP_STAMPS_DUMP file.
usage: stamps_split.py <dump> <label> [remainder]   (remainder: the plan splits half / quarter tiles)
The launch list is rebuilt from the lengths by the planner's rule (full tiles class after class, largest K first; then every
other tile by decreasing rows x (K + 4), stable in the order main, quarter, half classes, K descending)."""
import sys, pathlib
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import numpy as np
from tests.synth import make_config

dump, label = sys.argv[1], sys.argv[2]
split = len(sys.argv) > 3
seqs, cfg = make_config("cfg2")
lens = np.array([len(s) for s in seqs])
ROWS = 1024
k8 = (lens + 7) // 8
full = 0
per_k = {}
for k in sorted(np.unique(k8), reverse=True):
    cols = np.nonzero(k8 == k)[0]
    cols = cols[cols >= 1]
    halves, quarters, resid = [], [], []
    for c in range(0, len(cols), 2):
        span = int(cols[min(c + 1, len(cols) - 1)])
        full += span // ROWS
        r = span % ROWS
        if split:
            if r >= ROWS // 2:
                halves.append(ROWS // 2); r -= ROWS // 2
            if r >= ROWS // 4:
                quarters.append(ROWS // 4); r -= ROWS // 4
        if r:
            resid.append(r)
    resid.sort(reverse=True)
    per_k[int(k)] = (halves, quarters, resid)
others = []  # (work, insertion index, kind, rows)
if split:
    for k, (h, q, r) in per_k.items():
        for rows in q:
            others.append((rows * (k + 4), len(others), "quarter", rows))
        for rows in r:
            others.append((rows * (k + 4), len(others), "residual", rows))
    for k, (h, q, r) in per_k.items():
        for rows in h:
            others.append((rows * (k + 4), len(others), "half", rows))
else:
    for k, (h, q, r) in per_k.items():
        for rows in r:
            others.append((rows * (k + 4), len(others), "residual", rows))
others.sort(key=lambda x: (-x[0], x[1]))
kinds = np.array([o[2] for o in others])
rows_o = np.array([o[3] for o in others])
h = np.fromfile(dump, dtype=np.uint64)
n = len(h) // 7
c0 = h[2:3 * n:3].astype(np.int64)
c1 = h[3 * n:6 * n:3].astype(np.int64)
c2 = h[3 * n + 1:6 * n:3].astype(np.int64)
c3 = h[6 * n:7 * n].astype(np.int64)
steps = h[3 * n + 2:6 * n:3].astype(np.int64)
print(f"[{label}] {n} tiles in the dump; counted from the lengths: {full} full, {len(others)} other tiles")
assert n == full + len(others), "the dump is not the cfg2 bundle this script counts"
tot = (c3 - c0).sum()
def line(name, idx, rows):
    clk = (c3 - c0)[idx].sum()
    print(f"[{label}] {name}: {len(c0[idx])} tiles, {rows} rows, {clk / rows:.1f} clocks per row "
          f"(prologue {(c1 - c0)[idx].mean():.0f}, main loop {(c2 - c1)[idx].mean():.0f} = {(c2 - c1)[idx].sum() / steps[idx].sum():.2f} per step, "
          f"epilogue {(c3 - c2)[idx].mean():.0f} clocks per tile), {100.0 * clk / tot:.2f} % of the launch's tile clocks")
    return clk / rows
a = line("full tiles", np.arange(0, full), full * ROWS)
for kind in ("half", "quarter", "residual"):
    idx = full + np.nonzero(kinds == kind)[0]
    if len(idx):
        b = line(kind + " tiles", idx, int(rows_o[kinds == kind].sum()))
        print(f"[{label}] a row of a {kind} tile costs {b / a:.3f} x a row of a full tile")
b = line("all other tiles", np.arange(full, n), int(rows_o.sum()))
print(f"[{label}] a row of the other tiles costs {b / a:.3f} x a row of a full tile")
