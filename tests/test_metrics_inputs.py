"""On the device: the one structure-batch check of codlad_amd/metrics/_inputs.py refuses a wrong rank, an empty batch and
a wrong atom count at every entry point before anything is launched, and the geometry check and the relaxation of one
topology read the same device tensors.  Two structures of a three-residue topology (tests/test_metrics_inputs_host.py)."""
import pytest
import torch

from codlad_amd import _lib, metrics
from tests.test_metrics_inputs_host import NO_COUNT, entry_points, topology


@pytest.mark.gpu
def test_bad_structures_are_refused_before_any_launch_and_tables_are_shared(monkeypatch):
    top = topology()
    x = (torch.randn(2, top.n_atoms, 3, generator=torch.Generator().manual_seed(7)) * 3.0).cuda()
    calls = entry_points(top)
    real = _lib.lib
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "lib", lambda: pytest.fail("a refused input reached the library"))
        for name, call in calls.items():
            for what, bad in (("rank", x[0]), ("empty", x[:0]), ("count", x[:, :-1].contiguous())):
                if what == "count" and name in NO_COUNT:
                    continue
                with pytest.raises(ValueError):
                    call(bad, x)
    assert _lib.lib is real
    # every entry point takes the batch itself
    for name, call in calls.items():
        call(x, x)
    torch.cuda.synchronize()

    # geometry_check, then relax: one radius table and one exclusion CSR on the device, through the caches
    top = topology()
    geo = metrics.geometry_check(x, top)
    out = metrics.relax(x, top, n_iter=1)
    radius, excl_ptr, excl, bonds = top._geometry_tables[(2, "cuda:0")]
    tab = top._relax_tables[(2, "cuda:0")]
    assert tab is metrics._relax_tables_on(top, 2, x.device)
    assert radius.data_ptr() == tab["radius"].data_ptr()
    assert excl_ptr.data_ptr() == tab["excl_ptr"].data_ptr() == tab["pair_ptr"].data_ptr()
    assert excl.data_ptr() == tab["excl"].data_ptr() == tab["pair_j"].data_ptr()
    # and they are the right tables: the *_lists forms, which build their own, return the same bits
    host = metrics.relax_tables(top)
    lists = (host["radius"], bonds.cpu().long(), host["quads"])
    geo_l = metrics.geometry_check_lists(x, *lists[:2])
    out_l = metrics.relax_lists(x, *lists, fixed=host["fixed"], n_iter=1)
    assert torch.equal(geo["counts"], geo_l["counts"])
    assert torch.equal(geo["min_dist"].view(torch.int32), geo_l["min_dist"].view(torch.int32))
    assert torch.equal(out["xyz"].view(torch.int32), out_l["xyz"].view(torch.int32))
    assert torch.equal(out["trace_energy"].view(torch.int64), out_l["trace_energy"].view(torch.int64))
