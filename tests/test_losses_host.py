"""CPU-only checks of the loss evaluation's host side: the forward-process tables and the loss coefficient table against the
reference's extracted schedule values, the LossType mapping of create_diffusion, the refusals, and the float64 restatement
of the loss terms (tests/loss_cases.py) against the reference's own `.double()` evaluation in the g19 goldens."""
import numpy as np
import pytest
import torch

from codlad_amd import diffusion_and_flow as df
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps
from tests import cases
from tests import loss_cases as lc


def tables():
    return Tables(named_betas("linear", 1000), space_timesteps(1000, str(lc.T)))


def test_forward_process_tables_match_the_reference_bit_for_bit():
    g = np.load(cases.npz_path("g19_schedule_10"))
    tb = tables()
    for name in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod", "posterior_variance"):
        assert np.array_equal(getattr(tb, name), g[name]), name
    assert np.array_equal(1.0 - tb.alphas_cumprod, g["one_minus_alphas_cumprod"])
    # existing tables keep their values
    g1 = np.load(cases.npz_path("g1_schedule_10"))
    for name in ("betas", "sqrt_recip_alphas_cumprod", "posterior_mean_coef1", "posterior_log_variance_clipped"):
        assert np.array_equal(getattr(tb, name), g1[name]), name


def test_loss_coefficients_are_the_values_the_reference_extracts():
    ex = np.load(cases.npz_path("g19_schedule_10"))["extracted"]      # [9, T] fp32, _extract_into_tensor's `.float()`
    tb = tables()
    c = tb.loss_coefficients()
    assert c.dtype == np.float32 and c.shape == (lc.T, tb.LOSS_COLUMNS)
    for col, row in ((8, 0), (9, 1), (10, 2), (11, 3), (12, 4), (6, 5), (2, 6), (3, 7)):
        assert np.array_equal(c[:, col], ex[row]), (col, row)
    assert np.array_equal(c[:, :6], tb.step_coefficients()[:, :6]) and np.array_equal(c[:, 7], tb.step_coefficients()[:, 7])
    assert not c[:, 13:].any()
    large = tb.loss_coefficients(var_type="fixed_large", predict_xstart=True, clip_denoised=True)
    assert np.array_equal(large[:, 4], ex[8]) and np.array_equal(large[:, 6], ex[5])      # model / true log variance
    assert (large[:, 7] == 7).all()
    small = tb.loss_coefficients(var_type="fixed_small")
    assert np.array_equal(small[:, 4], ex[5]) and (small[:, 7] == 2).all()


def test_create_diffusion_maps_the_loss_type_as_the_reference():
    assert df.create_diffusion("10").loss_type is df.LossType.MSE
    assert df.create_diffusion("10", rescale_learned_sigmas=True).loss_type is df.LossType.RESCALED_MSE
    assert df.create_diffusion("10", use_kl=True).loss_type is df.LossType.RESCALED_KL
    assert df.create_diffusion("10", use_kl=True, rescale_learned_sigmas=True).loss_type is df.LossType.RESCALED_KL
    assert df.LossType.KL.is_vb() and df.LossType.RESCALED_KL.is_vb() and not df.LossType.MSE.is_vb()
    assert [m.name for m in df.LossType] == ["MSE", "RESCALED_MSE", "KL", "RESCALED_KL"]


def test_loss_entry_points_refuse_cpu_tensors_and_other_widths():
    d = df.create_diffusion("10")
    x = torch.zeros(2, 5, 3)
    t = torch.tensor([1, 2])
    model = lambda *a, **k: None          # noqa: E731  (never reached)
    for call in (lambda: d.q_sample(x, t, noise=x), lambda: d.q_mean_variance(x, t), lambda: d.q_posterior_mean_variance(x, x, t),
                 lambda: d._vb_terms_bpd(model, x, x, t), lambda: d.training_losses(model, x, t),
                 lambda: d.calc_bpd_loop(model, x)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()


@pytest.mark.parametrize("name", list(lc.LOSS_CASES))
def test_float64_restatement_reproduces_the_references_double_terms(name):
    L, B, seed, n_rep, kw, _loss_type, _kind, ts, _rs = lc.LOSS_CASES[name]
    g = np.load(cases.npz_path("g19_loss_" + name))
    _prot, _batch, _mask, x_start, noise = lc.inputs(L, B, seed, n_rep)
    x_start, noise = lc.stored_inputs(g, x_start, noise)
    px, var = lc.diffusion_flags(kw)
    assert tuple(g["t"]) == tuple(ts)
    got = lc.terms64(tables(), torch.from_numpy(g["model_out"]), x_start, torch.from_numpy(g["x_t"]), noise[0],
                     torch.tensor(ts), predict_xstart=px, var_type=var, clip_denoised=False)
    for k in ("kl", "nll", "vb", "mse", "xstart_mse", "eps_mse"):
        ref = torch.from_numpy(g["f64_" + k])
        assert ref.dtype == torch.float64
        # float64 rounding: sums of 3 L terms and a tanh / exp / log each
        assert torch.allclose(got[k], ref, rtol=1e-11, atol=0), (k, got[k], ref)


@pytest.mark.parametrize("name", list(lc.BPD_CASES))
def test_float64_restatement_reproduces_the_bound_loop(name):
    L, B, seed, kw, _kind, clip = lc.BPD_CASES[name]
    g = np.load(cases.npz_path("g19_" + name))
    _prot, _batch, _mask, x_start, eps = lc.inputs(L, B, seed, 1, n_steps=lc.T)
    x_start, eps = lc.stored_inputs(g, x_start, eps)
    px, var = lc.diffusion_flags(kw)
    tb = tables()
    for k, i in enumerate(range(lc.T - 1, -1, -1)):
        t = torch.full((x_start.shape[0],), i)
        got = lc.terms64(tb, torch.from_numpy(g["model_out"][k]), x_start, torch.from_numpy(g["x_t"][k]), eps[k], t,
                         predict_xstart=px, var_type=var, clip_denoised=clip)
        for key in ("vb", "xstart_mse", "eps_mse"):
            assert torch.allclose(got[key], torch.from_numpy(g["f64_" + key][k]), rtol=1e-11, atol=0), (i, key)
    # -1 - lv + exp(lv) cancels two unit-size numbers down to the result's 3e-5: float64 rounding is 1e-16 absolute
    assert torch.allclose(lc.prior64(tb, x_start), torch.from_numpy(g["f64_prior_bpd"]), rtol=0, atol=1e-15)
    # the golden's layout is the IDDPM release's: [N, T], column k = step T-1-k; the total is the row sum plus the prior
    assert g["vb"].shape == (x_start.shape[0], lc.T)
    assert np.array_equal(g["vb"], g["f32_vb"].T)
    assert np.allclose(g["total_bpd"], g["vb"].sum(1) + g["prior_bpd"], rtol=1e-6)
