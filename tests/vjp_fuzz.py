"""Shared by the reverse-mode fuzz tests (test_vjp_fuzz_host.py, test_gpu_vjp_fuzz.py): random programs of tests/fuzz.py with their
multivector leaves bound as inputs, their cotangents, the dual-number reference of vjp_dual_numpy.py per (item, slot), and the
bookkeeping of what was compared and what the domain rule left out.

C64 and C32 bound |gradient - reference| <= C eps scale per component.  They follow DESIGN.md section 11's rule: the next power of two
at least 4 x above the worst ratio measured ON THE CPU, of vjp_numpy's plain f64 / f32 evaluation of the VJP image to the longdouble
reference (test_vjp_fuzz_host.py prints those ratios); no GPU output went into them.
"""
import ctypes as C

import numpy as np

from gaast_amd import _lib
from fuzz import random_big_program, random_program, realise
from helpers import HipBackend
from vjp_dual_numpy import eval_dual
from vjp_numpy import EXPLICIT_LIMIT, GradeAbsent, Program, eval_desc

C64, C32 = 16, 16
EPS64, EPS32 = 2.0 ** -52, 2.0 ** -23
LEFT_OUT_CAP, SKIP_CAP = 0.15, 0.15


def bound_program(seed, batch, big=False):
    """(n, metric, build, rows): build() realises the program on the product's front end with every multivector leaf bound as an input;
    rows[slot] is [batch, row]; no rows: the program has no bound input"""
    n, metric, spec = (random_big_program if big else random_program)(seed)
    rows = {}
    realise(spec, HipBackend(), n, rows=rows, batch=batch)
    return n, metric, (lambda: realise(spec, HipBackend(), n, rows={}, batch=batch)), rows


def cotangent(seed, batch, out_len):
    return np.random.default_rng([seed, 77]).uniform(-1.0, 1.0, (batch, out_len))


_images = []   # kept alive: a desc points into its image


def vjp_image(d, slot):
    """(status, desc or None) of gaast_program_vjp"""
    img = C.c_void_p()
    st = _lib.lib().gaast_program_vjp(C.byref(d), slot, C.byref(img))
    if st:
        return st, None
    _images.append(img)
    return 0, _lib.lib().gaast_program_image_desc(img).contents


def explicit_program(build, metric):
    """vjp_numpy.Program of the forward image with explicit lists (the reference's input), and the spec that owns it"""
    spec = build().specialize(metric, materialize_limit=EXPLICIT_LIMIT)
    return Program(spec.program_desc()), spec


def panics(prog, rows):
    """the reference would panic on this program (a sum over unequal grade sets reaches a buffer without the grade)"""
    try:
        eval_desc(prog, {s: r[0] for s, r in rows.items()})
        return False
    except GradeAbsent:
        return True


class Tally:
    """What a test compared: worst ratio err / (eps scale), checks made and left out, programs run and skipped."""

    def __init__(self):
        self.worst, self.where = 0.0, None
        self.checked = self.left_out = self.programs = self.skipped = self.unbound = 0

    def compare(self, got, ref, g, eps, C, where, extra=0.0):
        """got: gradient row.  ref: vjp_dual_numpy.Dual.  Asserts |got - J g| <= (C + extra) eps scale per component (so exactly 0
        where scale is 0), unless the item is outside the domain."""
        if ref.outside:
            self.left_out += 1
            return
        want, scale = ref.vjp(g)
        self.check(np.asarray(got), want, scale, eps, C + extra, where)

    def check(self, got, want, scale, eps, C, where):
        err = np.abs(got.astype(np.longdouble) - want)
        ok = scale > 0
        ratio = float(np.max(err[ok] / (eps * scale[ok]), initial=0.0))
        if ratio > self.worst or not np.isfinite(ratio):
            self.worst, self.where = ratio, where
        self.checked += 1
        assert np.all(err <= C * eps * scale), f"ratio {ratio:.3g} > {C} (or a non-zero where the scale is 0): {where}\n" \
            f"got {got}\nwant {want.astype(np.float64)}\nscale {scale.astype(np.float64)}"

    def caps(self):
        assert self.checked > 0
        total = self.checked + self.left_out
        assert self.left_out <= LEFT_OUT_CAP * total, f"{self.left_out} of {total} checks left out"
        bound = self.programs - self.unbound
        assert self.skipped <= SKIP_CAP * bound, f"{self.skipped} of {bound} programs skipped"

    def merge(self, other):
        if other.worst > self.worst:
            self.worst, self.where = other.worst, other.where
        for k in ("checked", "left_out", "programs", "skipped", "unbound"):
            setattr(self, k, getattr(self, k) + getattr(other, k))

    def __str__(self):
        total = self.checked + self.left_out
        return (f"worst ratio {self.worst:.3f} ({self.where}); {self.checked} checks, {self.left_out} left out "
                f"({100.0 * self.left_out / max(total, 1):.2f} %); {self.programs} programs, {self.skipped} skipped, {self.unbound} without bound input")


def reference(prog, rows, item, slot, rounded=None, V=None):
    return eval_dual(prog, {s: r[item] for s, r in rows.items()}, slot, V=V, rounded=rounded)
