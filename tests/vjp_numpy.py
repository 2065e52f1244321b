"""A plain numpy evaluator of flat programs (gaast_program_desc), one item at a time, with eval.rs's in-place semantics.

Independent of the library's planner and kernels: it reads the node table as eval.rs does (store_in_cache / add_to_res) and is used
by the reverse-mode tests to evaluate forward programs and their VJP programs on the CPU.  Compact products are regenerated from
the library's own phase-3 rules only through explicit lists: a compact product node (a forward kind, or GAAST_PROD_ADJ_LEFT /
ADJ_RIGHT over one) is evaluated from the explicit list of a two-input product of that kind over the node's three grade sets,
specialised with a large materialisation limit and, for an adjoint kind, transposed here in forward order.

`dtype=np.float32` rounds every read and every operation result to f32 (the arithmetic of an f32 program); the default is f64.
"""
import ctypes as C
import math

import numpy as np

from gaast_amd import _lib

_CM = np.dtype([("lg", "<u4"), ("li", "<u4"), ("rg", "<u4"), ("ri", "<u4"), ("og", "<u4"), ("oi", "<u4"), ("c", "<f8")])
assert _CM.itemsize == C.sizeof(_lib.CompMul)
EXPLICIT_LIMIT = 1 << 24


class GradeAbsent(AssertionError):
    """A node adds a grade its buffer does not hold: where the reference panics (quirk Q5, sums of unequal grade sets)."""


def _layout(dim, mask):
    off, pos = {}, 0
    for k in range(64):
        if (mask >> k) & 1:
            off[k] = pos
            pos += math.comb(dim, k)
    return off, pos


def _offsets(dim, mask):
    """grade -> offset as an array (-1: grade absent), and the row length"""
    off, n = _layout(dim, mask)
    a = np.full(64, -1, dtype=np.int64)
    for k, o in off.items():
        a[k] = o
    return a, n


def _grades(mask):
    return [k for k in range(64) if (mask >> k) & 1]


_forward_lists = {}


def forward_list(n, metric, base, lmask, rmask, omask):
    """The explicit list (structured array, forward order) of the product of kind `base` of operands with grades lmask and rmask,
    restricted to the result grades omask: what phase 3 writes for that product with a large materialisation limit."""
    key = (n, tuple(metric), base, lmask, rmask, omask)
    if key not in _forward_lists:
        import gaast_amd as ga
        a, b = ga.mv(ga.Input(0, _grades(lmask), n)), ga.mv(ga.Input(1, _grades(rmask), n))
        e = {_lib.PROD_GEOMETRIC: lambda: a * b, _lib.PROD_OUTER: lambda: a ^ b, _lib.PROD_INNER: lambda: a & b,
             _lib.PROD_LCONTRACT: lambda: a << b, _lib.PROD_RCONTRACT: lambda: a >> b, _lib.PROD_REGRESSIVE: lambda: a.vee(b)}[base]()
        spec = e.gselect(_grades(omask)).specialize(list(metric), materialize_limit=EXPLICIT_LIMIT)
        d = spec.program_desc()
        found = [d.nodes[i] for i in range(d.n_nodes) if d.nodes[i].opcode == _lib.OP_PRODUCT and d.nodes[i].minimal_grade_mask]
        assert len(found) <= 1
        if found and found[0].n_comp_muls:
            assert found[0].comp_muls, "the list was not materialised"
            lst = _list_of(found[0])
            lst = lst[((omask >> lst["og"].astype(np.uint64)) & np.uint64(1)).astype(bool)]
        else:
            lst = np.zeros(0, dtype=_CM)
        _forward_lists[key] = lst
    return _forward_lists[key]


def _list_of(nd):
    return np.frombuffer(C.string_at(nd.comp_muls, int(nd.n_comp_muls) * _CM.itemsize), dtype=_CM).copy()


class _Node:
    __slots__ = ("opcode", "child0", "child1", "mask", "dim", "slot", "kind", "n_comp_muls", "lst")


class Program:
    """A flat program as plain data: read once from a gaast_program_desc, evaluated many times."""

    def __init__(self, d):
        self.n = d.vec_space_dim
        self.metric = [d.metric_diag[i] for i in range(self.n)]
        self.root = d.root
        self.inputs = []
        for s in range(d.n_inputs):
            ind = d.inputs[s]
            _, n = _layout(ind.storage_dim, ind.grade_mask)
            const = np.array([ind.const_row[i] for i in range(n)], dtype=np.float64) if ind.is_const else None
            self.inputs.append((ind.grade_mask, ind.storage_dim, bool(ind.is_const), const))
        self.nodes = []
        for i in range(d.n_nodes):
            s, nd = d.nodes[i], _Node()
            nd.opcode, nd.child0, nd.child1, nd.mask, nd.dim = s.opcode, s.child0, s.child1, s.minimal_grade_mask, s.vec_space_dim
            nd.slot, nd.kind, nd.n_comp_muls = s.input_slot, s.product_kind, int(s.n_comp_muls)
            nd.lst = _list_of(s) if s.opcode == _lib.OP_PRODUCT and s.comp_muls else None
            self.nodes.append(nd)
        self._entries = {}

    def user_slots(self):
        return [s for s, ind in enumerate(self.inputs) if not ind[2]]

    def row_len(self, slot):
        return _layout(self.inputs[slot][1], self.inputs[slot][0])[1]

    def buf_len(self, i):
        return _layout(self.nodes[i].dim, self.nodes[i].mask)[1]

    def out_len(self):
        return self.buf_len(self.root)

    def segment(self, res, k):
        """the slice of grade k in the buffer of node `res`"""
        off, _ = _layout(self.nodes[res].dim, self.nodes[res].mask)
        if k not in off:
            raise GradeAbsent("grade absent from result buffer")
        return slice(off[k], off[k] + math.comb(self.nodes[res].dim, k))

    def product_list(self, i):
        """(list in the roles left, right, result of the node's children and the node; forward order) of PRODUCT node i"""
        nd = self.nodes[i]
        if nd.lst is not None:
            return nd.lst
        if nd.n_comp_muls == 0:      # no list and nothing to regenerate: an empty product
            return np.zeros(0, dtype=_CM)
        assert nd.kind >= 0, "PRODUCT node has neither a list nor a kind"
        adj, base = nd.kind & ~7, nd.kind & 7
        m0, m1 = self.nodes[nd.child0].mask, self.nodes[nd.child1].mask
        if adj == 0:
            lst = forward_list(self.n, self.metric, base, m0, m1, nd.mask)
        elif adj == _lib.PROD_ADJ_LEFT:      # children (g, b), node = a: (l, r -> o, c) becomes (o, r -> l, c)
            f = forward_list(self.n, self.metric, base, nd.mask, m1, m0)
            lst = np.zeros(len(f), dtype=_CM)
            lst["lg"], lst["li"], lst["rg"], lst["ri"], lst["og"], lst["oi"], lst["c"] = f["og"], f["oi"], f["rg"], f["ri"], f["lg"], f["li"], f["c"]
        else:                                # children (g, a), node = b: (l, r -> o, c) becomes (o, l -> r, c)
            assert adj == _lib.PROD_ADJ_RIGHT
            f = forward_list(self.n, self.metric, base, m1, nd.mask, m0)
            lst = np.zeros(len(f), dtype=_CM)
            lst["lg"], lst["li"], lst["rg"], lst["ri"], lst["og"], lst["oi"], lst["c"] = f["og"], f["oi"], f["lg"], f["li"], f["rg"], f["ri"], f["c"]
        assert len(lst) == nd.n_comp_muls, (len(lst), nd.n_comp_muls)
        nd.lst = lst
        return lst

    def entries(self, i, res):
        """(left index, right index, result index, coefficient) arrays of PRODUCT node i adding into the buffer of node `res`"""
        key = (i, res)
        if key not in self._entries:
            nd, lst = self.nodes[i], self.product_list(i)
            lo, _ = _offsets(self.nodes[nd.child0].dim, self.nodes[nd.child0].mask)
            ro, _ = _offsets(self.nodes[nd.child1].dim, self.nodes[nd.child1].mask)
            oo, _ = _offsets(self.nodes[res].dim, self.nodes[res].mask)
            assert np.all(lo[lst["lg"]] >= 0) and np.all(ro[lst["rg"]] >= 0)
            if not np.all(oo[lst["og"]] >= 0):
                raise GradeAbsent("grade absent from result buffer")
            self._entries[key] = (lo[lst["lg"]] + lst["li"], ro[lst["rg"]] + lst["ri"], oo[lst["og"]] + lst["oi"], lst["c"].copy())
        return self._entries[key]

    def input_segments(self, i, res):
        """[(result start, input start, length)] of INPUT node i adding into the buffer of node `res` (slices zipped)"""
        nd = self.nodes[i]
        imask, sd = self.inputs[nd.slot][:2]
        ioff, _ = _layout(sd, imask)
        roff, _ = _layout(self.nodes[res].dim, self.nodes[res].mask)
        out = []
        for k in _grades(nd.mask & imask):
            if k not in roff:
                raise GradeAbsent("grade absent from result buffer")
            out.append((roff[k], ioff[k], min(math.comb(self.nodes[res].dim, k), math.comb(sd, k))))
        return out

    def flips(self, i):
        nd = self.nodes[i]
        return [k for k in _grades(nd.mask)
                if nd.opcode == _lib.OP_NEG or (nd.opcode == _lib.OP_REVERSE and k % 4 in (2, 3)) or (nd.opcode == _lib.OP_GINVOL and k % 2 == 1)]


def eval_desc(d, rows, dtype=np.float64):
    """d: a gaast_program_desc or a Program.  rows: {slot: 1-D row} for the non-const slots.  Returns the root's row."""
    p = d if isinstance(d, Program) else Program(d)
    nodes = p.nodes
    ins = {}
    for s, (imask, sd, is_const, const) in enumerate(p.inputs):
        if is_const:
            ins[s] = const.astype(dtype)
        elif s in rows:
            ins[s] = np.asarray(rows[s], dtype=np.float64).astype(dtype)
    cache = {}

    def store(i):
        if i in cache:
            return
        off, n = _layout(nodes[i].dim, nodes[i].mask)
        cache[i] = (np.zeros(n, dtype=dtype), off)
        add(i, i)

    def seg(res, k):
        off = cache[res][1]
        if k not in off:
            raise GradeAbsent("grade absent from result buffer")
        return slice(off[k], off[k] + math.comb(nodes[res].dim, k))

    def add(res, i):
        nd = nodes[i]
        if nd.mask == 0:
            return
        buf = cache[res][0]
        op = nd.opcode
        if op == _lib.OP_INPUT:
            row = ins[nd.slot]
            for ro, io, n in p.input_segments(i, res):
                buf[ro:ro + n] += row[io:io + n]
        elif op == _lib.OP_ADD:
            add(res, nd.child0)
            add(res, nd.child1)
        elif op in (_lib.OP_NEG, _lib.OP_REVERSE, _lib.OP_GINVOL):
            add(res, nd.child0)
            for k in p.flips(i):
                buf[seg(res, k)] *= -1
        elif op in (_lib.OP_SINV, _lib.OP_SSQRT):
            add(res, nd.child0)
            s = seg(res, 0).start
            with np.errstate(all="ignore"):
                buf[s] = dtype(1.0) / buf[s] if op == _lib.OP_SINV else np.sqrt(buf[s])
        elif op == _lib.OP_PROJ:
            add(res, nd.child0)
        elif op == _lib.OP_PRODUCT:
            store(nd.child0)
            store(nd.child1)
            li, ri, oi, c = p.entries(i, res)
            with np.errstate(all="ignore"):
                np.add.at(buf, oi, cache[nd.child0][0][li] * cache[nd.child1][0][ri] * c.astype(dtype))
        else:
            raise NotImplementedError(_lib.OP_NAMES[op])

    store(p.root)
    return cache[p.root][0]
