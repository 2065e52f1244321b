"""gaast_hip_linmap_*: outermorphisms of a linear map on batches of graded rows (kernels_linmap.hip.hpp), against numpy compounds."""
import ctypes as C

import numpy as np
import pytest

import gaast_amd as ga
from clifford_gram import blades_of_grade
from helpers import linmap_host_apply as host_apply

pytestmark = pytest.mark.gpu
PD = C.POINTER(C.c_double)
NP = {ga.F32: np.float32, ga.F64: np.float64}


def check(n, grades, batch, dtype, seed, orthogonal=False):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1, 1, (n, n))
    if orthogonal:
        m = np.linalg.qr(m)[0]
    rl = sum(len(blades_of_grade(n, k)) for k in grades)
    rows = rng.uniform(-1, 1, (batch, rl)).astype(NP[dtype])
    x = ga.DeviceMV.from_rows(n, grades, rows, dtype)
    y = ga.Outermorphism(m, dtype).apply(x)
    got = y.download_rows().astype(np.float64)
    want = host_apply(m, grades, rows)
    # norm-wise per row: |err|_2 <= c eps |C_k(M)|_2 |x|_2 on each grade; |C_k(M)|_2 <= |M|_2^k
    eps = 2.0 ** -52 if dtype == ga.F64 else 2.0 ** -23
    scale = max(1.0, np.linalg.norm(m, 2)) ** n * np.linalg.norm(rows.astype(np.float64), axis=1)
    err = np.linalg.norm(got - want, axis=1)
    assert (err <= 64 * eps * scale + 1e-300).all(), (err / scale).max()


@pytest.mark.parametrize("dtype", [ga.F32, ga.F64])
@pytest.mark.parametrize("n", [3, 5, 6, 8, 12])
def test_linmap_full_rows(n, dtype):
    for batch in (1, 37):
        check(n, list(range(n + 1)), batch, dtype, seed=n * 10 + batch)


@pytest.mark.parametrize("dtype", [ga.F32, ga.F64])
@pytest.mark.parametrize("n,grades", [(3, [1]), (5, [0, 2, 4]), (6, [1, 3, 5]), (8, [2, 3]), (12, [0, 1, 6, 12])])
def test_linmap_partial_masks(n, grades, dtype):
    check(n, grades, 65, dtype, seed=n)


@pytest.mark.parametrize("dtype", [ga.F32, ga.F64])
@pytest.mark.parametrize("n", [5, 8])
def test_linmap_large_batch(n, dtype):
    check(n, list(range(n + 1)), 65536 if n == 5 else 4099, dtype, seed=3, orthogonal=True)


@pytest.mark.parametrize("n", [5, 8])
def test_linmap_strided_torch_views(n):
    import torch
    rng = np.random.default_rng(n)
    m = rng.uniform(-1, 1, (n, n))
    grades = list(range(n + 1))
    rl = 1 << n
    dev = torch.device("cuda:0")
    big_in = torch.tensor(rng.uniform(-1, 1, (50, rl + 3)), dtype=torch.float64, device=dev)
    big_out = torch.zeros((50, rl + 5), dtype=torch.float64, device=dev)
    x = ga.DeviceMV.wrap_tensor(big_in[:, 1:1 + rl], n, grades)
    y = ga.DeviceMV.wrap_tensor(big_out[:, 2:2 + rl], n, grades)
    ga.Outermorphism(m, ga.F64).apply(x, y)
    torch.cuda.synchronize()
    ga.lib().gaast_hip_synchronize()
    got = big_out.cpu().numpy()
    want = host_apply(m, grades, big_in[:, 1:1 + rl].cpu().numpy())
    assert np.abs(got[:, 2:2 + rl] - want).max() <= 1e-12 * (1 + np.abs(want).max())
    assert not got[:, :2].any() and not got[:, 2 + rl:].any()     # nothing written outside the view


@pytest.mark.parametrize("dtype", [ga.F32, ga.F64])
@pytest.mark.parametrize("n", [5, 9])
def test_identity_is_a_bitwise_copy_and_q_qt_round_trips(n, dtype):
    rng = np.random.default_rng(1)
    grades = list(range(n + 1))
    rows = rng.uniform(-1, 1, (129, 1 << n)).astype(NP[dtype])
    x = ga.DeviceMV.from_rows(n, grades, rows, dtype)
    y = ga.Outermorphism(np.eye(n), dtype).apply(x)
    assert np.array_equal(y.download_rows(), rows)
    q = np.linalg.qr(rng.uniform(-1, 1, (n, n)))[0]
    z = ga.Outermorphism(q.T, dtype).apply(ga.Outermorphism(q, dtype).apply(x))
    tol = 1e-13 if dtype == ga.F64 else 1e-5
    assert np.abs(z.download_rows().astype(np.float64) - rows).max() <= tol


def test_linmap_refuses_mismatches():
    L = ga.lib()
    f = ga.Outermorphism(np.eye(4), ga.F64)
    x = ga.DeviceMV.alloc(4, [1, 2], 8, ga.F64)
    for bad in (ga.DeviceMV.alloc(4, [1], 8, ga.F64), ga.DeviceMV.alloc(5, [1, 2], 8, ga.F64),
                ga.DeviceMV.alloc(4, [1, 2], 9, ga.F64), ga.DeviceMV.alloc(4, [1, 2], 8, ga.F32)):
        assert L.gaast_hip_linmap_apply(f._h, x._h, bad._h) == 6
    assert L.gaast_hip_linmap_apply(f._h, x._h, x._h) == 6                           # in place: overlap
    import torch
    t = torch.zeros((9, 10 + 1), dtype=torch.float64, device="cuda:0")
    a = ga.DeviceMV.wrap_tensor(t[:8, :10], 4, [1, 2])
    b = ga.DeviceMV.wrap_tensor(t[1:9, :10], 4, [1, 2])
    assert L.gaast_hip_linmap_apply(f._h, a._h, b._h) == 6                           # overlapping views
    h = C.c_void_p()
    m = np.eye(15)
    assert L.gaast_hip_linmap_create(15, m.ctypes.data_as(PD), ga.F64, C.byref(h)) == 3   # beyond n = 14
    assert not h.value


def test_linmap_kernel_names_in_launches():
    g = np.array([[1.0, 0.3, 0.0], [0.3, -1.0, 0.2], [0.0, 0.2, 0.5]])
    a = ga.mv(ga.Input(0, [1], 3))
    b = ga.mv(ga.Input(1, [1, 2], 3))
    names = (a * b).specialize(ga.GramAlgebra(g)).launches()
    assert names[0].startswith("linmap[input 0") and "k_linmap_small<double>" in names[0]
    assert names[1].startswith("linmap[input 1")
    assert names[-1].startswith("linmap[result") and "k_linmap_small<double>" in names[-1]
    n = 8
    a = ga.mv(ga.Input(0, list(range(n + 1)), n))
    rng = np.random.default_rng(0)
    g = rng.uniform(-1, 1, (n, n))
    names = (a * a).specialize(ga.GramAlgebra(g + g.T), dtype=ga.F32).launches()
    assert "k_linmap_mfma<float>" in names[0] and "k_linmap_mfma<float>" in names[-1]
