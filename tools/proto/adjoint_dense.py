"""CPU prototype of the dense adjoints of the geometric product (reverse mode), checked against the Jacobian
of the bitmask form C[a ^ b] += s(a, b) m(a & b) A[a] B[b] (algebra.rs:73-83) for random diagonal metrics with negative, scaled
and null squares.

With Z the null vectors, m'(p) = 1 / m(p) off Z and 0 on Z, mn(j) the product of m over the non-null vectors of blade j,
rev(j) = (-1)^(|j|(|j|-1)/2) and R(a, b) = #{p in a, q in b, p > q} mod 2:
    dA[i] = P[i ^ Z],  P = G' *_{m'} B**,  G'[k] = G[k ^ Z],  B**[j] = rev(j) mn(j) (-1)^R(Z, j) B[j]
    dB[i] = Q[i ^ Z],  Q = A** *_{m'} G',  A**[j] = rev(j) mn(j) (-1)^R(j, Z) A[j]
i.e. a FORWARD geometric product in the metric m' with relabelled / re-signed / rescaled operands and a relabelled result: the
operand and output maps of the dense kernels.  Z empty is the non-degenerate identity dA = G *_{1/m} B*."""
import numpy as np


def R(a, b):
    c = 0
    q = 0
    while b >> q:
        if (b >> q) & 1:
            c += bin(a >> (q + 1)).count("1")
        q += 1
    return c & 1


def mprod(metric, blade):
    v = 1.0
    for p, g in enumerate(metric):
        if (blade >> p) & 1:
            v *= g
    return v


def gp(A, B, metric):
    N = len(A)
    C = np.zeros(N)
    for a in range(N):
        if A[a] == 0.0:
            continue
        for b in range(N):
            C[a ^ b] += (-1.0) ** R(a, b) * mprod(metric, a & b) * A[a] * B[b]
    return C


def adjoints_direct(G, A, B, metric):
    N = len(A)
    dA, dB = np.zeros(N), np.zeros(N)
    for a in range(N):
        for b in range(N):
            c = (-1.0) ** R(a, b) * mprod(metric, a & b)
            dA[a] += c * G[a ^ b] * B[b]
            dB[b] += c * G[a ^ b] * A[a]
    return dA, dB


def adjoints_dense(G, A, B, metric):
    n, N = len(metric), len(A)
    Z = sum(1 << p for p, g in enumerate(metric) if g == 0.0)
    mp = [0.0 if g == 0.0 else 1.0 / g for g in metric]
    nn = [1.0 if g == 0.0 else g for g in metric]
    rev = lambda j: (-1.0) ** ((bin(j).count("1") * (bin(j).count("1") - 1) // 2) % 2)
    Gp = np.array([G[k ^ Z] for k in range(N)])
    B2 = np.array([rev(j) * mprod(nn, j) * (-1.0) ** R(Z, j) * B[j] for j in range(N)])
    A2 = np.array([rev(j) * mprod(nn, j) * (-1.0) ** R(j, Z) * A[j] for j in range(N)])
    P, Q = gp(Gp, B2, mp), gp(A2, Gp, mp)
    return np.array([P[i ^ Z] for i in range(N)]), np.array([Q[i ^ Z] for i in range(N)])


def random_metric(rng, n):
    m = rng.choice([1.0, -1.0, 0.0, 2.0, -0.5, 1.5], size=n)
    return [float(x) for x in m]


def check(n_metrics=40, dims=(4, 5, 6, 7), seed=0):
    rng = np.random.default_rng(seed)
    worst = 0.0
    for n in dims:
        for t in range(n_metrics):
            metric = random_metric(rng, n)
            if t == 0:
                metric[0] = 0.0   # at least one null vector
            if t == 1:
                metric[0] = metric[-1] = 0.0
            N = 1 << n
            G, A, B = (rng.uniform(-1, 1, N) for _ in range(3))
            dA, dB = adjoints_direct(G, A, B, metric)
            eA, eB = adjoints_dense(G, A, B, metric)
            err = max(np.max(np.abs(dA - eA)), np.max(np.abs(dB - eB))) / (1.0 + np.max(np.abs(dA)) + np.max(np.abs(dB)))
            worst = max(worst, err)
            assert err <= 1e-12, (n, metric, err)
    return worst


if __name__ == "__main__":
    print("max relative error", check())
