"""CPU checks of the ensemble analysis: the host reference the GPU tests compare against (tests/ensemble_ref.py) agrees
with `metrics.superposed_rmsd` and excludes reflections, the C ABI declares and exports the new entry points and rejects
bad arguments before any HIP call, and `compute_div` on CPU tensors is bit for bit the parent's formula."""
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics as gm
from tests import ensemble_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("codlad_ens_moments", "codlad_ens_pair_msd", "codlad_ens_apply", "codlad_ens_pairwise")


def test_reference_agrees_with_superposed_rmsd_on_random_pairs():
    """Two float64 SVD routes over the same centred data (numpy / torch): equal up to the rounding of their sums,
    far inside the bound the device is held to."""
    for n in (3, 4, 65, 257, 1000):
        a, b = er.batch(7, n, 11 + n)
        for k in range(7):
            ref = er.kabsch(a[k], b[k])
            want = gm.superposed_rmsd(torch.from_numpy(a[k].copy()), torch.from_numpy(b[k].copy())) ** 2
            assert abs(max(ref["msd"], 0.0) - want) <= er.msd_bound(n, ref["e0n"]), (n, k)
            moved = a[k].astype(np.float64) @ ref["R"].T + ref["t"]
            assert np.linalg.det(ref["R"]) > 0
            assert abs(er.plain_msd(moved, b[k]) - ref["msd"]) <= 1e-9 * ref["e0n"], (n, k)


def test_mirror_image_of_a_chiral_blob_is_not_superposable():
    """z -> -z of a 3-D blob: an improper map would give 0; the proper optimum leaves 2 s3 / n (s3 the smallest singular
    value of the covariance), far above rounding."""
    for n in (4, 65, 1000):
        for off in er.OFFSETS:
            a, b = er.make_pair("mirror", n, off, er.case_seed("mirror", n, off))
            ref = er.kabsch(a, b)
            assert ref["msd"] > 1e-3 * ref["e0n"], (n, off)
            assert np.linalg.det(ref["R"]) > 0


def test_rigid_copies_have_zero_msd_within_the_bound():
    """The rigid copy is rounded to fp32 after the motion, so its msd is not 0 but the rounding's: coordinates of
    magnitude M carry 2^-24 M each."""
    for n in er.SIZES:
        for off in er.OFFSETS:
            a, b = er.make_pair("rigid", n, off, er.case_seed("rigid", n, off))
            ref = er.kabsch(a, b)
            m = max(float(np.abs(a).max()), float(np.abs(b).max()))
            assert max(ref["msd"], 0.0) <= 3 * (2.0 ** -23 * m) ** 2 + er.msd_bound(n, ref["e0n"]), (n, off, ref["msd"])


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(codlad_ens_[a-z0-9_]+)\s*\(", header))
    assert declared == set(ENTRY_POINTS)
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced by these calls
    p = buf.ctypes.data
    assert lib.codlad_ens_moments(None, 1, 4, None, 0, p, None) < 0 and b"null pointer" in lib.codlad_last_error()
    assert lib.codlad_ens_moments(p, 1, 4, None, 0, None, None) < 0
    assert lib.codlad_ens_moments(p, 0, 4, None, 0, p, None) < 0
    assert lib.codlad_ens_moments(p, 1, -4, None, 0, p, None) < 0
    assert lib.codlad_ens_moments(p, 1, 4, None, 3, p, None) < 0            # a count without a list
    assert lib.codlad_ens_moments(p, 1, 4, p, 0, p, None) < 0               # a list without a count
    assert lib.codlad_ens_moments(p, 1, 4, p, -1, p, None) < 0
    assert lib.codlad_ens_pair_msd(None, p, 1, p, p, 1, 4, None, 0, p, 1, 1, p, None, None) < 0
    assert lib.codlad_ens_pair_msd(p, p, 1, p, p, 1, 4, None, 0, None, 1, 1, p, None, None) < 0
    assert lib.codlad_ens_pair_msd(p, p, 1, p, p, 1, 4, None, 0, p, 1, 1, None, None, None) < 0
    assert lib.codlad_ens_pair_msd(p, p, 1, p, p, 1, 4, None, 0, p, 0, 1, p, None, None) < 0
    assert lib.codlad_ens_pair_msd(p, p, -1, p, p, 1, 4, None, 0, p, 1, 1, p, None, None) < 0
    assert lib.codlad_ens_pair_msd(p, p, 1, p, p, 1, 0, None, 0, p, 1, 1, p, None, None) < 0
    assert lib.codlad_ens_apply(None, p, 1, 4, p, None) < 0
    assert lib.codlad_ens_apply(p, p, 1, 4, None, None) < 0
    assert lib.codlad_ens_apply(p, p, -1, 4, p, None) < 0
    assert lib.codlad_ens_apply(p, p, 1, 0, p, None) < 0
    assert lib.codlad_ens_pairwise(None, p, 2, 1, 4, None, 0, 0, p, None) < 0
    assert lib.codlad_ens_pairwise(p, None, 2, 1, 4, None, 0, 0, p, None) < 0
    assert lib.codlad_ens_pairwise(p, p, 0, 1, 4, None, 0, 0, p, None) < 0
    assert lib.codlad_ens_pairwise(p, p, 2, -1, 4, None, 0, 0, p, None) < 0
    assert lib.codlad_ens_pairwise(p, p, 65536, 65536, 4, None, 0, 0, p, None) < 0     # G * F overflows the grid
    assert lib.codlad_ens_pairwise(p, p, 2, 1, 4, None, 2, 0, p, None) < 0


def test_python_wrappers_reject_cpu_tensors_and_bad_selections():
    a = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        gm.superposed_rmsd_batch(a, a)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        gm.pairwise_rmsd(a[None])
    with pytest.raises(ValueError, match="outside"):
        gm._selection([0, 5], 5, "cpu")
    with pytest.raises(ValueError, match="empty"):
        gm._selection([], 5, "cpu")


def test_compute_div_on_cpu_tensors_is_the_parent_formula_bit_for_bit():
    """The CPU path is the yardstick of the device path and must not move: restated here as the parent commit has it."""
    def rmsd(a, b):
        a = a.to(torch.float64) - a.to(torch.float64).mean(0)
        b = b.to(torch.float64) - b.to(torch.float64).mean(0)
        u, sv, vt = torch.linalg.svd((a.t() @ b).cpu())
        d = torch.sign(torch.linalg.det(u @ vt))
        e0 = float((a * a).sum() + (b * b).sum())
        return (max(e0 - 2.0 * float(sv[0] + sv[1] + d * sv[2]), 0.0) / a.shape[0]) ** 0.5

    for dtype in (torch.float32, torch.float64):
        g = torch.Generator().manual_seed(5)
        base = torch.randn(3, 97, 3, generator=g, dtype=dtype) * 5
        gen = [base + 0.4 * torch.randn(3, 97, 3, generator=g, dtype=dtype) for _ in range(4)]
        ref = base + 0.7
        mean_gen = torch.stack(gen).mean(0)
        to_ref = [rmsd(x[p], ref[p]) for x in gen for p in range(3)]
        to_mean = [rmsd(x[p], mean_gen[p]) for x in gen for p in range(3)]
        want = 1.0 - (sum(to_mean) / len(to_mean)) / (sum(to_ref) / len(to_ref))
        assert gm.compute_div(gen, ref) == want
        assert gm.compute_div([x.numpy() for x in gen], ref.numpy()) == want
