"""The 3 x 3 eigensolver, directly and without a GPU (matrices: tests/eigh3_families.py).

Three statements, each about a different pair:

  * csrc/eigh3.h compiled for the HOST (tests/eigh3_host_shim.hip, the library's floating-point flags) equals the oracle's
    independent restatement orc_eigh3 bit for bit on every family -- also outside LAPACK's unscaled domain, where the two must
    still be the same function;
  * orc_eigh3 equals the installed NumPy's np.linalg.eigh (LAPACK dsyevd) inside the domain, eigenvector signs included;
  * orc_eigh3 is as accurate as np.linalg.eigh against 50-digit arithmetic (mpmath), within a factor of 4.

On eigenvector signs.  For integer-valued symmetric matrices, for real ones with exact zeros off the diagonal, and for
strongly graded ones (`range`), LAPACK's column signs are not a function of the matrix alone: the same LAPACK source built
with another compiler or BLAS keeps a last-bit residue where this restatement has an exact zero, or rounds a cancelled
tridiagonal entry the other way; a rotation then starts from the other side and columns come out negated -- to within 1e-10
the same eigenvectors.  The oracle's own source built with fused multiply-adds shows it against itself (0.4 - 0.8 % of such
matrices), and shows none on generic, PSD, near-degenerate and low-rank input (eigh3_families.UP_TO_SIGN).  So on `intsym`,
`negzero`, `realzero`, `range` and the integer part of `scaled` columns are compared UP TO SIGN, every matrix with a simple
spectrum still compared and held to the same tolerance, and the number of flipped columns is printed; everywhere else a
flipped sign is a failure.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigh3_families as F
from conftest import ROOT
from oracle import oracle as O

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
W_TOL = 1e-14   # |w - w_lapack| <= W_TOL max|w_lapack|: the constant of test_eigh3_matches_lapack_including_signs
V_TOL = 1e-13   # max|v - v_lapack| <= V_TOL / gap wherever the relative gap exceeds GAP_MIN
GAP_MIN = 1e-6


def bits_equal(w1, v1, w2, v2):
    """Per matrix: all twelve outputs have the same bit pattern."""
    return (w1.view(np.uint64) == w2.view(np.uint64)).all(axis=1) & (v1.view(np.uint64) == v2.view(np.uint64)).all(axis=(1, 2))


def has_nonfinite(w, v):
    return (~np.isfinite(w)).any(axis=1) | (~np.isfinite(v)).any(axis=(1, 2))


@pytest.fixture(scope="module")
def host_eigh3(tmp_path_factory):
    """eigh3_lower built for the host with the flags of csrc/Makefile: f(a (m, 3, 3)) -> (w, v)."""
    if HIPCC is None:
        pytest.skip("no hipcc")
    so = str(tmp_path_factory.mktemp("eigh3_host") / "libeigh3_host.so")
    r = subprocess.run([HIPCC, "--offload-host-only", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                        "-I", os.path.join(ROOT, "shot_fpfh_amd", "csrc"), os.path.join(ROOT, "tests", "eigh3_host_shim.hip"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    lib.eigh3_host.restype = None
    lib.eigh3_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]

    def solve(a):
        lo = F.lower(a)
        w, v = np.zeros((lo.shape[0], 3)), np.zeros((lo.shape[0], 3, 3))
        lib.eigh3_host(lo.ctypes.data, lo.shape[0], w.ctypes.data, v.ctypes.data)
        return w, v

    return solve


@pytest.fixture(scope="module")
def oracle_results():
    """{family: (w, v)} from orc_eigh3, computed once."""
    return {name: O.eigh3_batch(a) for name, a in F.families().items()}


def test_families_are_what_they_say():
    f = F.families()
    assert list(f) == list(F.INSIDE) + ["outside", "nonfinite"]
    assert 35_000 <= sum(a.shape[0] for a in f.values()) <= 45_000
    assert np.signbit(f["negzero"][f["negzero"] == 0.0]).any()
    span = np.abs(f["range"]).max(axis=(1, 2))
    assert (span > 0.1).sum() > 500 and (span < 1e-50).sum() > 100
    for zeros in F.ZERO_PATTERNS:  # all eight zero patterns occur in the real-valued family exactly as asked
        a = f["realzero"]
        hit = np.all((a[:, [1, 2, 2], [0, 0, 1]] == 0.0) == np.array(zeros), axis=1)
        assert hit.sum() == a.shape[0] // 8
    assert np.array_equal(F.lower(np.arange(9.0).reshape(1, 3, 3)), [[0.0, 3.0, 6.0, 4.0, 7.0, 8.0]])


def test_host_build_of_the_header_equals_the_oracle_bit_for_bit(host_eigh3, oracle_results):
    counts = {}
    for name, a in F.families().items():
        w, v = host_eigh3(a)
        wo, vo = oracle_results[name]
        if name == "nonfinite":  # fmax and an `if` treat NaN differently: only "both return, something is non-finite"
            counts[name] = (int((has_nonfinite(w, v) & has_nonfinite(wo, vo)).sum()), a.shape[0])
        else:
            counts[name] = (int(bits_equal(w, v, wo, vo).sum()), a.shape[0])
    print("host build == oracle, bit for bit (nonfinite: both have a non-finite output):", counts)
    assert all(got == m for got, m in counts.values()), counts


def lapack_deviation(a, w, v):
    """Against np.linalg.eigh per matrix: eigenvalue error / max|w|, the relative gap, max|dv| with signs, max|dv| up to a
    sign per column, and the number of columns that are closer to the negated one."""
    w_np, v_np = np.linalg.eigh(a)
    big = np.abs(w_np).max(axis=1)
    safe = np.where(big > 0.0, big, 1.0)
    dw = np.abs(w - w_np).max(axis=1) / safe
    gap = np.where(big > 0.0, np.minimum(w_np[:, 1] - w_np[:, 0], w_np[:, 2] - w_np[:, 1]) / safe, 0.0)
    plus, minus = np.abs(v - v_np).max(axis=1), np.abs(v + v_np).max(axis=1)  # (m, 3): per column
    return dw, gap, plus.max(axis=1), np.minimum(plus, minus).max(axis=1), (minus < plus).sum(axis=1)


def test_oracle_equals_this_machines_lapack_inside_the_domain(oracle_results):
    f = F.families()
    report = {}
    for name in F.INSIDE:
        a = f[name]
        w, v = oracle_results[name]
        dw, gap, dv_signed, dv_unsigned, flips = lapack_deviation(a, w, v)
        structured = F.scaled_is_structured() if name == "scaled" else np.full(a.shape[0], name in F.UP_TO_SIGN)
        simple = gap > GAP_MIN
        dv = np.where(structured, dv_unsigned, dv_signed)  # every simple-spectrum matrix is compared, one way or the other
        report[name] = dict(m=a.shape[0], simple=int(simple.sum()), dw=float(dw.max()), dv_gap=float((dv * gap)[simple].max(initial=0.0)),
                            flipped_columns=int(flips[simple & structured].sum()), flipped_matrices=int((flips[simple & structured] > 0).sum()))
        print(name, report[name])
        assert dw.max() <= W_TOL, (name, dw.max())
        worst = int(np.argmax(np.where(simple, dv * gap, 0.0)))
        assert np.all((dv * gap)[simple] <= V_TOL), (name, worst, a[worst].tolist(), dv[worst], gap[worst])
        assert flips[simple & ~structured].sum() == 0  # (the flipped share of the others is informational: it is NumPy's build's)


def test_oracle_is_as_accurate_as_lapack_against_exact_arithmetic(oracle_results):
    """200 matrices per family inside the domain, at 50 digits: eigenvalue error, residual max_k |A v_k - w_k v_k| (both
    relative to max|a|) and |V^T V - I|.  Bound: 4 x the worst np.linalg.eigh shows on the same matrices, and never more than
    1e-14.  (4: the restatements scale a block by divide-then-multiply where dlascl multiplies once.)"""
    mp = pytest.importorskip("mpmath")
    f = F.families()
    with mp.workdps(50):
        for name in F.INSIDE:
            a_all = f[name]
            pick = np.linspace(0, a_all.shape[0] - 1, min(200, a_all.shape[0])).astype(int)
            w_np, v_np = np.linalg.eigh(a_all[pick])
            worst = {"oracle": [0.0, 0.0, 0.0], "numpy": [0.0, 0.0, 0.0]}
            for j, i in enumerate(pick):
                A = mp.matrix(np.tril(a_all[i]).tolist())
                A = A + A.T - mp.diag([A[k, k] for k in range(3)])
                scale = mp.mpf(float(np.abs(a_all[i]).max())) or mp.mpf(1)
                exact = sorted(mp.eigsy(A, eigvals_only=True))
                for who, w, v in (("oracle", oracle_results[name][0][i], oracle_results[name][1][i]), ("numpy", w_np[j], v_np[j])):
                    W, V = [mp.mpf(float(x)) for x in w], mp.matrix(v.tolist())
                    e_val = max(abs(W[k] - exact[k]) for k in range(3)) / scale
                    e_res = max(mp.norm(A * V[:, k] - W[k] * V[:, k]) for k in range(3)) / scale
                    e_orth = mp.mnorm(V.T * V - mp.eye(3), "f")
                    worst[who] = [max(x, float(y)) for x, y in zip(worst[who], (e_val, e_res, e_orth))]
            print(f"{name}: eigenvalue / residual / orthogonality  oracle {worst['oracle']}  numpy {worst['numpy']}")
            for got, ref, what in zip(worst["oracle"], worst["numpy"], ("eigenvalues", "residual", "orthogonality")):
                assert got <= min(4.0 * ref, 1e-14), (name, what, got, ref)
