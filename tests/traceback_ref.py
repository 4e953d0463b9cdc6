"""The alignment contract of include/seqalign_hip.h ("alignments for chosen pairs") restated in plain Python: full tables with
the reference's recurrences and border values (src/bio/method/nw.c, ga.c, sw.c), the tie rule, the run-length CIGAR and the
mirror for a > b.  Shares no code with the library; slow and literal on purpose (short sequences only).

align_pair(scoring, seq_a, seq_b, a_index, b_index) -> dict(score, a_begin, a_end, b_begin, b_end, columns, identities, cigar)
with cigar a list of (length, op) and op one of "M", "I" (a residue of a only), "D" (a residue of b only).
rescore(...) is what "the alignment has this score" means.

align_pair(..., flipped_ties=True) walks the same tables with the OTHER order among equally good moves (NW: up, diagonal,
left; Gotoh / SW in state M: X, Y, diagonal): an alignment of the same score that breaks the contract wherever there was a
tie.  The tests count with it how many of their pairs a device with another tie order could not pass; nothing else uses it.
`tabs` takes the result of tables(...) for the pair in its canonical orientation, so that both walks share one fill."""
from __future__ import annotations

SCORE_MIN = -(1 << 30)
NW, GA, SW = 0, 1, 2


def _codes(scoring, seq: bytes) -> list[int]:
    return [int(scoring.lut[ch]) for ch in seq]


def _sim(scoring, lo_code: int, hi_code: int) -> int:
    """S of a cell as the score kernels index the matrix: NW sub[lo][hi], Gotoh / SW sub[hi][lo]"""
    if scoring.method == NW:
        return int(scoring.sub[lo_code * 24 + hi_code])
    return int(scoring.sub[hi_code * 24 + lo_code])


def tables(scoring, lo: list[int], hi: list[int]):
    """M (H for NW), X, Y as (m + 1) x (n + 1) lists, rows = lo, columns = hi"""
    m, n = len(lo), len(hi)
    g, o, e = scoring.gap_pen, scoring.gap_opn, scoring.gap_ext
    M = [[0] * (n + 1) for _ in range(m + 1)]
    X = [[SCORE_MIN] * (n + 1) for _ in range(m + 1)]
    Y = [[SCORE_MIN] * (n + 1) for _ in range(m + 1)]
    if scoring.method == NW:
        for c in range(n + 1):
            M[0][c] = c * g
        for r in range(m + 1):
            M[r][0] = r * g
    elif scoring.method == GA:
        for c in range(1, n + 1):
            X[0][c] = max(M[0][c - 1] + o, X[0][c - 1] + e)
            M[0][c] = X[0][c]
        for r in range(1, m + 1):
            Y[r][0] = max(M[r - 1][0] + o, Y[r - 1][0] + e)
            M[r][0] = Y[r][0]
    sub, nw, sw = [int(v) for v in scoring.sub], scoring.method == NW, scoring.method == SW
    for r in range(1, m + 1):
        a = lo[r - 1]
        Mr, Mp, Xr, Yr, Yp = M[r], M[r - 1], X[r], Y[r], Y[r - 1]
        for c in range(1, n + 1):
            b = hi[c - 1]
            if nw:
                Mr[c] = max(Mr[c - 1] + g, Mp[c] + g, Mp[c - 1] + sub[a * 24 + b])
                continue
            sd = Mp[c - 1] + sub[b * 24 + a]
            x = max(Mr[c - 1] + o, Xr[c - 1] + e)
            y = max(Mp[c] + o, Yp[c] + e)
            Xr[c], Yr[c] = x, y
            Mr[c] = max(sd, x, y, 0) if sw else max(sd, x, y)
    return M, X, Y


def canonical(scoring, seq_a: bytes, seq_b: bytes, a_index: int, b_index: int):
    """(lo, hi): the codes of the row and of the column sequence"""
    if a_index > b_index:
        return _codes(scoring, seq_b), _codes(scoring, seq_a)
    return _codes(scoring, seq_a), _codes(scoring, seq_b)


def align_pair(scoring, seq_a: bytes, seq_b: bytes, a_index: int, b_index: int, flipped_ties: bool = False, tabs=None) -> dict:
    assert a_index != b_index
    flip = a_index > b_index
    lo, hi = canonical(scoring, seq_a, seq_b, a_index, b_index)
    m, n = len(lo), len(hi)
    M, X, Y = tabs if tabs is not None else tables(scoring, lo, hi)
    g, o = scoring.gap_pen, scoring.gap_opn
    r, c = m, n
    ops = []  # end first, canonical orientation: "I" consumes lo, "D" consumes hi
    if scoring.method == SW:
        best = max(max(row[1:]) for row in M[1:])
        if best == 0:
            return dict(score=0, a_begin=0, a_end=0, b_begin=0, b_end=0, columns=0, identities=0, cigar=[])
        r, c = next((i, j) for i in range(1, m + 1) for j in range(1, n + 1) if M[i][j] == best)
        score = best
    else:
        score = M[m][n]
    r_end, c_end = r, c
    ident = 0
    if scoring.method == NW and flipped_ties:
        while (r, c) != (0, 0):
            if r > 0 and M[r][c] == M[r - 1][c] + g:
                ops.append("I")
                r -= 1
            elif r > 0 and c > 0 and M[r][c] == M[r - 1][c - 1] + _sim(scoring, lo[r - 1], hi[c - 1]):
                ops.append("M")
                ident += lo[r - 1] == hi[c - 1]
                r, c = r - 1, c - 1
            else:
                ops.append("D")
                c -= 1
    elif scoring.method == NW:
        while (r, c) != (0, 0):
            if r > 0 and c > 0 and M[r][c] == M[r - 1][c - 1] + _sim(scoring, lo[r - 1], hi[c - 1]):
                ops.append("M")
                ident += lo[r - 1] == hi[c - 1]
                r, c = r - 1, c - 1
            elif r > 0 and M[r][c] == M[r - 1][c] + g:
                ops.append("I")
                r -= 1
            else:
                ops.append("D")
                c -= 1
    else:
        state = "M"
        while True:
            if state == "M":
                if scoring.method == SW and M[r][c] == 0:
                    break
                if (r, c) == (0, 0):
                    break
                diagonal = r > 0 and c > 0 and M[r][c] == M[r - 1][c - 1] + _sim(scoring, lo[r - 1], hi[c - 1])
                if flipped_ties and M[r][c] in (X[r][c], Y[r][c]):
                    diagonal = False
                if diagonal:
                    ops.append("M")
                    ident += lo[r - 1] == hi[c - 1]
                    r, c = r - 1, c - 1
                    continue
                state = "X" if M[r][c] == X[r][c] else "Y"
            if state == "X":
                ops.append("D")
                state = "M" if X[r][c] == M[r][c - 1] + o else "X"
                c -= 1
            else:
                ops.append("I")
                state = "M" if Y[r][c] == M[r - 1][c] + o else "Y"
                r -= 1
            assert r >= 0 and c >= 0
    ops.reverse()
    if flip:
        ops = [{"M": "M", "I": "D", "D": "I"}[op] for op in ops]
    cigar = []
    for op in ops:
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    lo_span, hi_span = (r, r_end), (c, c_end)
    a_span, b_span = (hi_span, lo_span) if flip else (lo_span, hi_span)
    return dict(score=score, a_begin=a_span[0], a_end=a_span[1], b_begin=b_span[0], b_end=b_span[1], columns=len(ops),
                identities=ident, cigar=cigar)
