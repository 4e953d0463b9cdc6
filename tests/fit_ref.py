"""The fit contract of include/seqalign_hip.h ("queries fitted inside database sequences") restated in plain Python: full tables,
the end cell, the walk, the run-length CIGAR.  Shares no code with the library or with tests/traceback_ref.py; literal on purpose.

The database sequence is the row sequence (r = 0 .. m), the query the column sequence (c = 0 .. n).  The tables are the method's
(NW: one table with a linear gap; Gotoh: M, X from the left, Y from above) with column 0 of M set to 0 in every row.

fit_pair(scoring, db_seq, query_seq) -> dict(score, db_begin, db_end, identities, columns, cigar, plateau): cigar a list of (length, op),
"M" a residue of each, "I" a residue of the query only, "D" a residue of the database sequence only (the record layout of the
hits: a = the query, b = the database sequence).
rescore(scoring, db_seq, query_seq, result) prices that CIGAR as the alignment contract prices an alignment.
global_score(scoring, db_codes, query_codes) is the plain global recurrence of the method, for the brute force over substrings."""
from __future__ import annotations

NEG = -(1 << 30)  # SCORE_MIN of the reference
NW, GA = 0, 1


def encode(scoring, seq: bytes) -> list:
    return [int(scoring.lut[ch]) for ch in seq]


def row0(scoring, c: int) -> int:
    """M[0][c] of the method: the query against nothing"""
    if scoring.method == NW:
        return c * scoring.gap_pen
    if c == 0:
        return 0
    o, e = scoring.gap_opn, scoring.gap_ext
    return max(o, NEG + e) + (c - 1) * max(o, e)


def _table(scoring):
    """S[d][q]: the substitution value of a database residue code against a query residue code, as the method indexes the matrix"""
    sub = [int(v) for v in scoring.sub]
    if scoring.method == NW:
        return [[sub[d * 24 + q] for q in range(24)] for d in range(24)]
    return [[sub[q * 24 + d] for q in range(24)] for d in range(24)]


def fill(scoring, db: list, qy: list, free_column: bool = True):
    """(M, X, Y), each (m + 1) x (n + 1).  free_column=False gives the method's own global tables."""
    assert scoring.method in (NW, GA), "fit is defined for NW and Gotoh"
    m, n = len(db), len(qy)
    g, o, e = scoring.gap_pen, scoring.gap_opn, scoring.gap_ext
    nw = scoring.method == NW
    S = _table(scoring)
    M = [[0] * (n + 1) for _ in range(m + 1)]
    X = [[NEG] * (n + 1) for _ in range(m + 1)]
    Y = [[NEG] * (n + 1) for _ in range(m + 1)]
    for c in range(n + 1):
        M[0][c] = row0(scoring, c)
    for r in range(1, m + 1):
        M[r][0] = 0 if free_column else row0(scoring, r)
    for r in range(1, m + 1):
        Sa = S[db[r - 1]]
        Mr, Mu, Xr, Yr, Yu = M[r], M[r - 1], X[r], Y[r], Y[r - 1]
        for c in range(1, n + 1):
            diag = Mu[c - 1] + Sa[qy[c - 1]]
            if nw:
                Mr[c] = max(Mr[c - 1] + g, Mu[c] + g, diag)
            else:
                x = max(Mr[c - 1] + o, Xr[c - 1] + e)
                y = max(Mu[c] + o, Yu[c] + e)
                Xr[c], Yr[c] = x, y
                Mr[c] = max(diag, x, y)
    return M, X, Y


def global_score(scoring, db: list, qy: list) -> int:
    return fill(scoring, db, qy, free_column=False)[0][len(db)][len(qy)]


def fit_codes(scoring, db: list, qy: list, flipped_ties: bool = False, last_end_row: bool = False, tabs=None) -> dict:
    """the contract's result, plus `plateau`: the number of rows r with M[r][n] equal to the maximum of column n.
    The two switches exist for the sensitivity of tests only (what ANOTHER rule would give on the same tables), both off by default:
    flipped_ties walks with the other order among equally good moves (NW: up before diagonal before left; Gotoh: X, then Y, before
    diagonal when leaving M -- the open / extend test unchanged), last_end_row takes the largest row among equal maxima of column n.
    tabs = fill(scoring, db, qy): one fill serves several walks."""
    m, n = len(db), len(qy)
    M, X, Y = fill(scoring, db, qy) if tabs is None else tabs
    g, o = scoring.gap_pen, scoring.gap_opn
    S = _table(scoring)
    # end cell: the largest M of column n, the smallest row on a tie; row 0 takes part
    end = 0
    for r in range(1, m + 1):
        if M[r][n] > M[end][n]:
            end = r
        elif last_end_row and M[r][n] == M[end][n]:  # (the other rule)
            end = r
    plateau = sum(1 for r in range(m + 1) if M[r][n] == M[end][n])
    r, c, state = end, n, "M"
    ops = []  # end first
    ident = 0
    while c > 0:
        if r == 0:
            ops.append("I")  # a residue of the query only
            c -= 1
            state = "M"
            continue
        if flipped_ties and scoring.method == NW and M[r][c] == M[r - 1][c] + g:  # (the other order: up first)
            ops.append("D")
            r -= 1
            continue
        if flipped_ties and scoring.method != NW and state == "M" and M[r][c] in (X[r][c], Y[r][c]):  # (the other order: X, then Y, first)
            state = "X" if M[r][c] == X[r][c] else "Y"
        if scoring.method == NW:
            if M[r][c] == M[r - 1][c - 1] + S[db[r - 1]][qy[c - 1]]:
                ops.append("M")
                ident += db[r - 1] == qy[c - 1]
                r, c = r - 1, c - 1
            elif M[r][c] == M[r - 1][c] + g:
                ops.append("D")
                r -= 1
            else:
                ops.append("I")
                c -= 1
            continue
        if state == "M":
            if M[r][c] == M[r - 1][c - 1] + S[db[r - 1]][qy[c - 1]]:
                ops.append("M")
                ident += db[r - 1] == qy[c - 1]
                r, c = r - 1, c - 1
                continue
            state = "X" if M[r][c] == X[r][c] else "Y"
        if state == "X":
            ops.append("I")
            state = "M" if X[r][c] == M[r][c - 1] + o else "X"
            c -= 1
        else:
            ops.append("D")
            state = "M" if Y[r][c] == M[r - 1][c] + o else "Y"
            r -= 1
    ops.reverse()
    cigar = []
    for op in ops:
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + 1, op)
        else:
            cigar.append((1, op))
    return dict(score=M[end][n], db_begin=r, db_end=end, identities=ident, columns=len(ops), cigar=cigar, plateau=plateau)


def fit_pair(scoring, db_seq: bytes, query_seq: bytes, flipped_ties: bool = False, last_end_row: bool = False, tabs=None) -> dict:
    return fit_codes(scoring, encode(scoring, db_seq), encode(scoring, query_seq), flipped_ties, last_end_row, tabs)


def rescore(scoring, db_seq: bytes, query_seq: bytes, res: dict) -> int:
    """S over the M columns plus, per gap run of length L, NW: L g; Gotoh: open + (L - 1) max(open, extend)"""
    db, qy = encode(scoring, db_seq), encode(scoring, query_seq)
    S = _table(scoring)
    r, c, total = res["db_begin"], 0, 0
    for length, op in res["cigar"]:
        if op == "M":
            for _ in range(length):
                total += S[db[r]][qy[c]]
                r, c = r + 1, c + 1
            continue
        if scoring.method == NW:
            total += length * scoring.gap_pen
        else:
            total += scoring.gap_opn + (length - 1) * max(scoring.gap_opn, scoring.gap_ext)
        if op == "I":
            c += length
        else:
            r += length
    assert r == res["db_end"] and c == len(qy), "the CIGAR does not cover the query and the database span"
    return total


def pid(identities: int, columns: int, m: int, n: int, denom: int) -> int:
    """the value rule of "percent identity of every pair": parts per million, floor; INT32_MIN for D <= 0"""
    num = identities * 1000000
    if denom == 0:
        d = columns
    elif denom == 1:
        d = min(m, n)
    elif denom == 2:
        d = max(m, n)
    else:
        d, num = m + n, 2 * num
    return -(1 << 31) if d <= 0 else num // d
