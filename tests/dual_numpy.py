"""Independent numpy reference of the complements and the regressive product, on blade bitmasks.

Blades are bitmasks S over n bits, ~S the complement of S in n bits, par(A, B) the parity of the number of pairs
(i in A, j in B, i > j):

    dual(e_S)   = (-1)^par(S, ~S) e_~S      right complement: e_S ^ dual(e_S) = I
    undual(e_S) = (-1)^par(~S, S) e_~S      left complement, the inverse of dual
    a v b       = undual(dual(a) ^ dual(b))

Everything here is computed from these three lines by counting pairs; nothing is shared with gaast_amd/csrc.  Rows are the
library's graded rows: grades ascending, ascending bitmask within a grade.
"""
import functools

import numpy as np


def par(a, b, n):
    """parity of #{(i in a, j in b): i > j}"""
    c = 0
    for i in range(n):
        if (a >> i) & 1:
            c += bin(b & ((1 << i) - 1)).count("1")
    return c & 1


@functools.lru_cache(maxsize=None)
def blades(n, k):
    """bitmasks of grade k in component order"""
    return tuple(m for m in range(1 << n) if bin(m).count("1") == k)


def row_blades(n, grades):
    out = []
    for k in sorted(grades):
        out.extend(blades(n, k))
    return out


def dual_sign(n, s):
    return -1.0 if par(s, ~s & ((1 << n) - 1), n) else 1.0


def undual_sign(n, s):
    return -1.0 if par(~s & ((1 << n) - 1), s, n) else 1.0


def wedge_blades(a, b, n):
    """e_a ^ e_b = sign e_{a|b}, or 0 when they share a vector"""
    if a & b:
        return 0.0, 0
    return (-1.0 if par(a, b, n) else 1.0), a | b


def vee_blades(a, b, n):
    """e_a v e_b by the definition, one complement at a time"""
    full = (1 << n) - 1
    s, w = wedge_blades(~a & full, ~b & full, n)
    if s == 0.0:
        return 0.0, 0
    s *= dual_sign(n, a) * dual_sign(n, b) * undual_sign(n, w)
    return s, ~w & full


# ---- on rows -------------------------------------------------------------------------------------------------------------
def complement_rows(n, grades, rows, undual=False, out_grades=None):
    """rows [B, len(grades' row)] -> (rows of the mirrored grades, those grades); 0.0 + (+-x) like the library's one rounding"""
    og = sorted(n - k for k in grades) if out_grades is None else sorted(out_grades)
    src_idx, dst_idx, negate, out_len = _complement_map(n, tuple(sorted(grades)), tuple(og), bool(undual))
    out = np.zeros((rows.shape[0], out_len), dtype=rows.dtype)
    x = rows[:, src_idx]
    out[:, dst_idx] = out[:, dst_idx] + np.where(negate[None, :], -x, x)
    return out, og


def add_complement(acc, n, grades, rows, undual=False):
    """acc + (+-rows) component by component, as a complement arm adds into a buffer that already holds acc (acc has the mirrored
    grades): one rounding, and the signed zeros of IEEE addition"""
    og = sorted(n - k for k in grades)
    src_idx, dst_idx, negate, out_len = _complement_map(n, tuple(sorted(grades)), tuple(og), bool(undual))
    assert acc.shape[1] == out_len
    out = acc.copy()
    x = rows[:, src_idx]
    out[:, dst_idx] = acc[:, dst_idx] + np.where(negate[None, :], -x, x)
    return out


@functools.lru_cache(maxsize=None)
def _complement_map(n, grades, og, undual):
    src = row_blades(n, grades)
    dst = {m: i for i, m in enumerate(row_blades(n, og))}
    full = (1 << n) - 1
    src_idx, dst_idx, negate = [], [], []
    for j, s in enumerate(src):
        t = ~s & full
        if t in dst:
            src_idx.append(j)
            dst_idx.append(dst[t])
            negate.append((undual_sign(n, s) if undual else dual_sign(n, s)) < 0)
    return np.array(src_idx, dtype=np.int64), np.array(dst_idx, dtype=np.int64), np.array(negate, dtype=bool), len(dst)


def vee_list(n, lgrades, rgrades, wanted=None):
    """The comp-mul list of a v b in order T4: (k_left, left index, k_right, right index, grade, index, coeff)"""
    return list(_vee_list(n, tuple(sorted(lgrades)), tuple(sorted(rgrades)), None if wanted is None else tuple(sorted(wanted))))


@functools.lru_cache(maxsize=None)
def _vee_list(n, lgrades, rgrades, wanted):
    out = []
    for kl in sorted(lgrades):
        for kr in sorted(rgrades):
            g = kl + kr - n
            if g < 0 or (wanted is not None and g not in wanted):
                continue
            res_index = {m: i for i, m in enumerate(blades(n, g))}
            for li, a in enumerate(blades(n, kl)):
                for ri, b in enumerate(blades(n, kr)):
                    s, r = vee_blades(a, b, n)
                    if s != 0.0:
                        out.append((kl, li, kr, ri, g, res_index[r], s))
    return out


def _offsets(n, grades):
    off, pos = {}, 0
    for k in sorted(grades):
        off[k] = pos
        pos += len(blades(n, k))
    return off, pos


def vee_rows(n, lgrades, lrows, rgrades, rrows, out_grades, sequential=False, absolute=False):
    """a v b per item.  sequential: summed entry by entry in list order in the rows' dtype, (l * r) * c then the add, as eval.rs:82
    does (the bits of GAAST_FLAG_EXACT_ORDER); else in float64.  absolute: sum |terms| (error bounds)."""
    lst = vee_list(n, lgrades, rgrades, set(out_grades))
    lo, _ = _offsets(n, lgrades)
    ro, _ = _offsets(n, rgrades)
    oo, olen = _offsets(n, out_grades)
    dt = np.dtype(lrows.dtype if sequential else np.float64)
    L, R = lrows.astype(dt), rrows.astype(dt)
    B = max(L.shape[0], R.shape[0])
    out = np.zeros((B, olen), dtype=dt)
    for kl, li, kr, ri, g, oi, c in lst:
        term = (L[:, lo[kl] + li] * R[:, ro[kr] + ri]) * dt.type(c)
        if absolute:
            term = np.abs(term)
        out[:, oo[g] + oi] = out[:, oo[g] + oi] + term
    return out


def vee_rows_transposed(n, lgrades, rgrades, out_grades, cot, other, wrt_left, absolute=False):
    """J^T cot of a v b with respect to the left (other = b rows) or right (other = a rows) operand, float64.
    absolute: sum |terms| (error bounds)."""
    lst = vee_list(n, lgrades, rgrades, set(out_grades))
    lo, llen = _offsets(n, lgrades)
    ro, rlen = _offsets(n, rgrades)
    oo, _ = _offsets(n, out_grades)
    cot, other = cot.astype(np.float64), other.astype(np.float64)
    if absolute:
        cot, other = np.abs(cot), np.abs(other)
    B = max(cot.shape[0], other.shape[0])
    out = np.zeros((B, llen if wrt_left else rlen))
    for kl, li, kr, ri, g, oi, c in lst:
        c = abs(c) if absolute else c
        if wrt_left:
            out[:, lo[kl] + li] += c * cot[:, oo[g] + oi] * other[:, ro[kr] + ri]
        else:
            out[:, ro[kr] + ri] += c * cot[:, oo[g] + oi] * other[:, lo[kl] + li]
    return out


def transpose_list(lst, right):
    """The transposed list the library builds for reverse mode: (l, r -> o, c) becomes (o, r -> l, c) for the left operand and
    (l, o -> r, c) for the right one, forward order kept, ordered stably by result component."""
    out = []
    for kl, li, kr, ri, g, oi, c in lst:
        out.append((kl, li, g, oi, kr, ri, c) if right else (g, oi, kr, ri, kl, li, c))
    return sorted(out, key=lambda m: (m[4], m[5]))


def permutation_check(n):
    """every (grade, index) -> (n - grade, C(n, grade) - 1 - index): used by the index-rule test"""
    full = (1 << n) - 1
    for k in range(n + 1):
        src, dst = blades(n, k), blades(n, n - k)
        for i, s in enumerate(src):
            yield k, i, dst.index(~s & full)
