"""A plain numpy evaluator of flat programs (gaast_program_desc), one item at a time, with eval.rs's in-place semantics.

Independent of the library's planner and kernels: it reads the node table as eval.rs does (store_in_cache / add_to_res) and is used
by the reverse-mode tests to evaluate forward programs and their VJP programs on the CPU.  Compact products are regenerated from
the library's own phase-3 rules only through explicit lists: programs given to it must carry explicit lists (the default
materialisation limit does that for small algebras).
"""
import math

import numpy as np

from gaast_amd import _lib


def _layout(dim, mask):
    off, pos = {}, 0
    for k in range(64):
        if (mask >> k) & 1:
            off[k] = pos
            pos += math.comb(dim, k)
    return off, pos


def eval_desc(d, rows):
    """rows: {slot: 1-D f64 row} for the non-const slots.  Returns the root's row."""
    nodes = [d.nodes[i] for i in range(d.n_nodes)]
    ins = {}
    for s in range(d.n_inputs):
        ind = d.inputs[s]
        off, n = _layout(ind.storage_dim, ind.grade_mask)
        if ind.is_const:
            ins[s] = (np.array([ind.const_row[i] for i in range(n)], dtype=np.float64), ind.storage_dim, ind.grade_mask)
        else:
            ins[s] = (np.asarray(rows[s], dtype=np.float64), ind.storage_dim, ind.grade_mask)
    cache = {}

    def store(i):
        if i in cache:
            return
        nd = nodes[i]
        off, n = _layout(nd.vec_space_dim, nd.minimal_grade_mask)
        cache[i] = (np.zeros(n), nd.vec_space_dim, nd.minimal_grade_mask, off)
        add(i, i)

    def seg(res, k):
        buf, dim, mask, off = cache[res]
        assert k in off, "grade absent from result buffer"
        return slice(off[k], off[k] + math.comb(dim, k))

    def add(res, i):
        nd = nodes[i]
        gs = nd.minimal_grade_mask
        if gs == 0:
            return
        buf = cache[res][0]
        op = nd.opcode
        if op == _lib.OP_INPUT:
            row, sd, imask = ins[nd.input_slot]
            ioff, _ = _layout(sd, imask)
            for k in range(64):
                if (gs >> k) & 1 and (imask >> k) & 1:
                    s = seg(res, k)
                    n = min(s.stop - s.start, math.comb(sd, k))
                    buf[s.start:s.start + n] += row[ioff[k]:ioff[k] + n]
        elif op == _lib.OP_ADD:
            add(res, nd.child0)
            add(res, nd.child1)
        elif op in (_lib.OP_NEG, _lib.OP_REVERSE, _lib.OP_GINVOL):
            add(res, nd.child0)
            for k in range(64):
                if not (gs >> k) & 1:
                    continue
                flip = op == _lib.OP_NEG or (op == _lib.OP_REVERSE and k % 4 in (2, 3)) or (op == _lib.OP_GINVOL and k % 2 == 1)
                if flip:
                    buf[seg(res, k)] *= -1.0
        elif op in (_lib.OP_SINV, _lib.OP_SSQRT):
            add(res, nd.child0)
            s = seg(res, 0)
            buf[s.start] = 1.0 / buf[s.start] if op == _lib.OP_SINV else math.sqrt(buf[s.start])
        elif op == _lib.OP_PROJ:
            add(res, nd.child0)
        elif op == _lib.OP_PRODUCT:
            store(nd.child0)
            store(nd.child1)
            assert nd.comp_muls, "numpy evaluator: explicit lists only"
            L, R = cache[nd.child0], cache[nd.child1]
            for e in range(nd.n_comp_muls):
                m = nd.comp_muls[e]
                lv = L[0][L[3][m.left_grade] + m.left_index]
                rv = R[0][R[3][m.right_grade] + m.right_index]
                buf[seg(res, m.result_grade).start + m.result_index] += lv * rv * m.coeff
        else:
            raise NotImplementedError("exp / log")

    store(d.root)
    return cache[d.root][0]
