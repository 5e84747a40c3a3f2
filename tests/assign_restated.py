"""Restatement of include/effdet_assign.h in plain integers, written from the header: the fp32 quantiser (NumPy float32, every operation
rounded once), a Hungarian solver of its own (the classic potentials form on the matrix padded with one private "stay unmatched" column
per line -- not the device's successive-shortest-path search over rows), brute force over all matchings for small problems, and
second_best(): the best total among the matchings that differ from the optimum.

A problem is the integer weight matrix W [rows][cols] (0 = the pair is not admissible).  Everything works per connected component of
the admissible graph, so that cap-sized problems made of small components stay cheap."""
import numpy as np

SCALE_BITS = 20
MAX_ROWS, MAX_COLS = 256, 128
_BIG = 1 << 40                                                                     # a forbidden pair: never taken, a line can always stay unmatched at 0


def weights(sim, gate):
    """sim [R, C] float32, gate -> int64 [R, C]: max(1, rint(min(sim - gate, 1) * 2^20)) where sim > gate (an fp32 compare), else 0"""
    sim, gate = np.asarray(sim, dtype=np.float32), np.float32(gate)
    with np.errstate(invalid='ignore'):
        ok = sim > gate                                                            # NaN: False
        d = np.minimum(np.where(ok, sim, gate) - gate, np.float32(1.0)).astype(np.float32)
        q = np.rint((d * np.float32(1 << SCALE_BITS)).astype(np.float32)).astype(np.int64)   # rint: ties to even
    return np.where(ok, np.maximum(q, 1), 0)


def _hungarian(cost):
    """cost [n, m] int64, n <= m -> for every line i the column it takes, minimising the sum (every line is assigned)"""
    n, m = cost.shape
    inf = np.iinfo(np.int64).max // 4
    u, v = np.zeros(n + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    p, way = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(m + 1, inf, dtype=np.int64), np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            idx = np.nonzero(used)[0]
            u[p[idx]] += delta
            v[idx] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = np.zeros(n, dtype=np.int64)
    for j in range(1, m + 1):
        if p[j]:
            out[p[j] - 1] = j - 1
    return out


def _solve_block(W):
    """One dense block -> (total, {row: col}).  Lines = the shorter side; each line may take its private zero column instead."""
    R, C = W.shape
    if R < C:
        t, m = _solve_block(W.T)
        return t, {r: c for c, r in m.items()}
    cost = np.full((C, R + C), _BIG, dtype=np.int64)                               # line = column c of W
    cost[:, :R] = np.where(W.T > 0, -W.T, _BIG)
    cost[np.arange(C), R + np.arange(C)] = 0
    take = _hungarian(cost)
    match = {int(take[c]): c for c in range(C) if take[c] < R}
    return int(sum(W[r, c] for r, c in match.items())), match


def components(W):
    """-> list of (rows, cols) of the connected components of the admissible graph that hold an edge"""
    W = np.asarray(W)
    R, C = W.shape
    seen_r, seen_c, out = np.zeros(R, dtype=bool), np.zeros(C, dtype=bool), []
    adm = W > 0
    for r0 in range(R):
        if seen_r[r0] or not adm[r0].any():
            continue
        rows, cols, todo = [], [], [('r', r0)]
        seen_r[r0] = True
        while todo:
            kind, k = todo.pop()
            if kind == 'r':
                rows.append(k)
                for c in np.nonzero(adm[k] & ~seen_c)[0]:
                    seen_c[c] = True
                    todo.append(('c', int(c)))
            else:
                cols.append(k)
                for r in np.nonzero(adm[:, k] & ~seen_r)[0]:
                    seen_r[r] = True
                    todo.append(('r', int(r)))
        out.append((sorted(rows), sorted(cols)))
    return out


def solve(W):
    """-> (total, {row: col}): a maximum-weight matching over the pairs with W > 0"""
    W = np.asarray(W, dtype=np.int64)
    total, match = 0, {}
    for rows, cols in components(W):
        t, m = _solve_block(W[np.ix_(rows, cols)])
        total += t
        match.update({rows[r]: cols[c] for r, c in m.items()})
    return total, match


def second_best(W):
    """The largest total among the matchings other than the optimum solve() returns (None when there is no other: an empty optimum).
    Complete: every admissible weight is >= 1, so a matching that keeps every optimal edge and adds one would beat the optimum; any
    other matching therefore lacks an optimal edge e, and the best of those is the optimum with e forbidden."""
    W = np.asarray(W, dtype=np.int64)
    total, best = solve(W)[0], None
    for rows, cols in components(W):
        sub = W[np.ix_(rows, cols)].copy()
        t, m = _solve_block(sub)
        for r, c in m.items():
            keep = sub[r, c]
            sub[r, c] = 0
            alt = total - t + _solve_block(sub)[0]
            sub[r, c] = keep
            best = alt if best is None else max(best, alt)
    return best


def brute(W):
    """The optimum by trying every matching (small problems only)"""
    W = np.asarray(W, dtype=np.int64)
    R, C = W.shape

    def go(r, used):
        if r == R:
            return 0
        best = go(r + 1, used)
        for c in range(C):
            if W[r, c] > 0 and not used & (1 << c):
                best = max(best, int(W[r, c]) + go(r + 1, used | (1 << c)))
        return best
    return go(0, 0)


def check_matching(W, row_to_col, col_to_row):
    """-> the sum of the weights of a returned matching, after asserting that the two maps are inverse and only admissible pairs appear"""
    W = np.asarray(W, dtype=np.int64)
    R, C = W.shape
    total = 0
    for r in range(R):
        c = int(row_to_col[r])
        assert -1 <= c < C, (r, c)
        if c >= 0:
            assert int(col_to_row[c]) == r and W[r, c] > 0, (r, c)
            total += int(W[r, c])
    for c in range(C):
        r = int(col_to_row[c])
        assert -1 <= r < R and (r < 0 or int(row_to_col[r]) == c), (c, r)
    return total
