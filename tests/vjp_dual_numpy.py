"""Forward-mode (dual-number) evaluation of a flat program in np.longdouble: the reference of the reverse-mode fuzz tests.

The same in-place structure as vjp_numpy.eval_desc (store / add, one buffer per product operand and for the root, flips and scalar
ops on the whole buffer so far), explicit lists only.  Every buffer carries four channels:

    v   the value                      vm  the value's magnitude: the same sums over absolute values
    t   tangents [D, len], one row per direction         tm  their magnitudes

    input            v += row, vm += |row|; for the differentiated slot t += V, tm += |V| (V = identity: the full Jacobian)
    neg / rev / ginvol   signs of v and t flip, magnitudes stay
    entry (l, r -> o, c) v[o] += c vl vr, vm[o] += |c| vml vmr, t[o] += c (tl vr + vl tr), tm[o] += |c| (tml vmr + vml tmr)
    SINV at s        v = 1/s, vm = vm/s^2, t = -t/s^2, tm = tm/s^2 + 2 vm tm/|s|^3
    SSQRT, r = sqrt s    v = r, vm = vm/(2r), t = t/(2r), tm = tm/(2r) + vm tm/(4 r^3)

tm bounds, to first order in eps, the rounding error any evaluation order of the derivative can make, divided by eps: it is the error
scale of the tests (|gradient - J^T g| <= C eps tm^T |g|).  At every scalar op kappa = vm/|s| is recorded; an item is OUTSIDE THE
DOMAIN if an s is not finite or 0, if s <= 0 at a sqrt, or if kappa > KAPPA_MAX (s is then mostly cancellation, and no first-order
bound holds).  Every other opcode (inv, dual, exp / log, gexp ...) raises: those have reference modules of their own.
"""
import numpy as np

from gaast_amd import _lib
from vjp_numpy import Program

LD = np.longdouble
KAPPA_MAX = 8.0


def _scatter_plan(p, i, res, oi):
    """(order, starts, targets): the entries of product i grouped by result component, for one reduceat per channel instead of an
    unbuffered np.add.at (the order of a longdouble sum is immaterial at the tests' eps)"""
    plans = p.__dict__.setdefault("_scatter_plans", {})
    if (i, res) not in plans:
        order = np.argsort(oi, kind="stable")
        targets, starts = np.unique(oi[order], return_index=True)
        plans[i, res] = (order, starts, targets)
    return plans[i, res]


class Dual:
    """Result of eval_dual.  value [len]; J, scale [D, len] (direction-major: J[d] = dF . V[d]); outside: the domain rule; kappa: the
    largest vm/|s| met."""

    def __init__(self, value, J, scale, outside, kappa):
        self.value, self.J, self.scale, self.outside, self.kappa = value, J, scale, outside, kappa

    def vjp(self, g):
        """(J^T g, its error scale) per direction, for a cotangent row g"""
        g = np.asarray(g, dtype=np.float64).astype(LD)
        return self.J @ g, self.scale @ np.abs(g)


def eval_dual(d, rows, wrt, V=None, rounded=None):
    """d: a gaast_program_desc or a vjp_numpy.Program with explicit lists.  rows: {slot: row} of the non-const slots.  wrt: the slot
    differentiated.  V: [D, row length of wrt] directions (default: the identity).  rounded: a dtype (np.float32) every input row and
    constant row is rounded to first, as a program of that dtype reads them."""
    p = d if isinstance(d, Program) else Program(d)
    nodes = p.nodes

    def read(x):
        x = np.asarray(x, dtype=np.float64)
        return (x.astype(rounded) if rounded is not None else x).astype(LD)
    ins = {s: read(const if is_const else rows[s]) for s, (_, _, is_const, const) in enumerate(p.inputs) if is_const or s in rows}
    V = np.eye(p.row_len(wrt), dtype=LD) if V is None else np.asarray(V, dtype=np.float64).astype(LD)
    absV = np.abs(V)
    D = V.shape[0]
    cache = {}
    state = {"outside": False, "kappa": 0.0}

    def store(i):
        if i in cache:
            return
        n = p.buf_len(i)
        cache[i] = (np.zeros(n, LD), np.zeros(n, LD), np.zeros((D, n), LD), np.zeros((D, n), LD))
        add(i, i)

    def add(res, i):
        nd = nodes[i]
        if nd.mask == 0:
            return
        v, vm, t, tm = cache[res]
        op = nd.opcode
        if op == _lib.OP_INPUT:
            row = ins[nd.slot]
            for ro, io, n in p.input_segments(i, res):
                v[ro:ro + n] += row[io:io + n]
                vm[ro:ro + n] += np.abs(row[io:io + n])
                if nd.slot == wrt:
                    t[:, ro:ro + n] += V[:, io:io + n]
                    tm[:, ro:ro + n] += absV[:, io:io + n]
        elif op == _lib.OP_ADD:
            add(res, nd.child0)
            add(res, nd.child1)
        elif op in (_lib.OP_NEG, _lib.OP_REVERSE, _lib.OP_GINVOL):
            add(res, nd.child0)
            for k in p.flips(i):
                s = p.segment(res, k)
                v[s] *= -1
                t[:, s] *= -1
        elif op == _lib.OP_PROJ:
            add(res, nd.child0)
        elif op in (_lib.OP_SINV, _lib.OP_SSQRT):
            add(res, nd.child0)
            k = p.segment(res, 0).start
            s, sm, st, stm = v[k], vm[k], t[:, k].copy(), tm[:, k].copy()
            bad = not np.isfinite(s) or s == 0 or (op == _lib.OP_SSQRT and s < 0)
            with np.errstate(all="ignore"):
                kappa = float(sm / abs(s)) if not bad else np.inf
                state["kappa"] = max(state["kappa"], kappa)
                if bad or not kappa <= KAPPA_MAX:
                    state["outside"] = True
                if op == _lib.OP_SINV:
                    v[k], vm[k] = 1 / s, sm / (s * s)
                    t[:, k] = -st / (s * s)
                    tm[:, k] = stm / (s * s) + 2 * sm * stm / abs(s) ** 3
                else:
                    r = np.sqrt(s)
                    v[k], vm[k] = r, sm / (2 * r)
                    t[:, k] = st / (2 * r)
                    tm[:, k] = stm / (2 * r) + sm * stm / (4 * r ** 3)
        elif op == _lib.OP_PRODUCT:
            assert nd.lst is not None or nd.n_comp_muls == 0, "dual reference: explicit lists only"
            store(nd.child0)
            store(nd.child1)
            li, ri, oi, c = p.entries(i, res)
            if not len(c):
                return
            c = c.astype(LD)
            ac = np.abs(c)
            lv, lvm, lt, ltm = cache[nd.child0]
            rv, rvm, rt, rtm = cache[nd.child1]
            order, starts, targets = _scatter_plan(p, i, res, oi)
            with np.errstate(all="ignore"):
                for buf, terms in ((v, c * lv[li] * rv[ri]), (vm, ac * lvm[li] * rvm[ri]),
                                   (t, c * (lt[:, li] * rv[ri] + lv[li] * rt[:, ri])),
                                   (tm, ac * (ltm[:, li] * rvm[ri] + lvm[li] * rtm[:, ri]))):
                    buf[..., targets] += np.add.reduceat(terms[..., order], starts, axis=-1)
        else:
            raise NotImplementedError("dual reference: " + _lib.OP_NAMES[op])

    store(p.root)
    v, vm, t, tm = cache[p.root]
    outside = state["outside"] or not (np.all(np.isfinite(t)) and np.all(np.isfinite(tm)))
    return Dual(v, t, tm, outside, state["kappa"])
