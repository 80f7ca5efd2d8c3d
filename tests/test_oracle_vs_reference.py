"""The oracle restatement against the reference on README-sized unets and beyond: the reference's outputs for the weights and inputs of
tests/reference_cases.py are recorded in tests/golden/reference_*.pt (python -m oracle.make_golden --reference-outputs, where the
reference's tree is present); these tests recompute the same cases with the oracle and this package's modules and compare."""
import pytest
import torch

import reference_cases as rc
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo


@pytest.fixture(scope="module")
def ref_unet():
    return rc.load_fixture("unet")


@pytest.fixture(scope="module")
def ref_unet3d():
    return rc.load_fixture("unet3d")


@pytest.fixture(scope="module")
def ref_sampler():
    return rc.load_fixture("sampler")


@pytest.mark.parametrize("name", list(rc.UNET_FORWARD), ids=list(rc.UNET_FORWARD))
def test_unet_forward(name, ref_unet):
    kw = rc.UNET_FORWARD[name]
    sd, x, t, te, extra = rc.unet_forward_case(kw)
    with torch.no_grad():
        for cdp, r in zip((0.0, 1.0), ref_unet[f"forward/{name}"]):
            o = uo.unet_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=cdp, **extra)
            assert torch.allclose(r, o, atol=1e-5), (r - o).abs().max()


def test_state_dict_layout_is_interchangeable(ref_unet):
    """The drop-in Unet must load a reference state_dict strictly (same keys, shapes, order)."""
    from imagen_pytorch_amd.unet import Unet

    for kw, ref in zip(rc.LAYOUT_CONFIGS, ref_unet["layout"]):
        ours = Unet(**kw)
        assert [k for k, _ in ref] == list(ours.state_dict().keys())
        ours.load_state_dict({k: torch.zeros(shape) for k, shape in ref})


@pytest.mark.parametrize("cond_ch,self_cond,mode", list(rc.SAMPLER.values()), ids=list(rc.SAMPLER))
def test_sampler_small_cascade(cond_ch, self_cond, mode, ref_sampler):
    name = next(k for k, v in rc.SAMPLER.items() if v == (cond_ch, self_cond, mode))
    unets, te, extra = rc.sampler_case(cond_ch, self_cond, mode)
    torch.manual_seed(123)  # the CPU RNG stream the reference sampled from: the oracle draws in the reference's order
    got = so.imagen_sample(unets, (16, 32), te, timesteps=4, cond_scale=3., return_all=True, resize_mode=mode, **extra)
    ref = ref_sampler[f"cascade/{name}"]
    assert len(ref) == len(got)
    for a, b in zip(ref, got):
        assert torch.allclose(a, b, atol=5e-4), (a - b).abs().max()


def test_unet3d_forward_readme_config(ref_unet3d):
    """SURVEY §8(f) NEXT-2 groundwork: oracle/unet3d_oracle.py vs the reference's `Unet3D` at the README video config's structure
    (`Unet3D(dim = 64, dim_mults = (1, 2, 4, 8))`, README.md:587; here dim 32 and an 8-frame 16x16 clip to keep the CPU test
    short), with temporal strides and the identity-initialised temporal layers randomised."""
    from oracle import unet3d_oracle as u3

    sd, x, t, te = rc.unet3d_readme_case()
    with torch.no_grad():
        for cdp, r in zip((0.0, 1.0), ref_unet3d["readme"]):
            o = u3.unet3d_forward(sd, rc.UNET3D_README, x, t, text_embeds=te, cond_drop_prob=cdp)
            assert r.abs().mean() > 0.05
            assert torch.allclose(r, o, atol=1e-4, rtol=1e-4), (r - o).abs().max()


@pytest.mark.parametrize("lowres", [False, True], ids=["base", "lowres"])
@pytest.mark.parametrize("prompts", ["pre", "post", "both"])
def test_unet3d_forward_with_prompt_frames(lowres, prompts, ref_unet3d):
    """Unet3D.forward(cond_video_frames=, post_cond_video_frames=) of the reference vs the oracle's restatement (iv.py:1682-1718,
    1933-1939), including the reference's frame order for succeeding frames and the low-res clip it extends for final_conv."""
    from oracle import unet3d_oracle as u3

    kw, sd, x, t, te, extra = rc.unet3d_prompt_case(lowres, prompts)
    with torch.no_grad():
        for cdp, r in zip((0.0, 1.0), ref_unet3d[f"prompt/{prompts}-{lowres}"]):
            o = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=cdp, **extra)
            assert r.shape == x.shape and r.abs().mean() > 0.05
            assert torch.allclose(r, o, atol=1e-4, rtol=1e-4), (r - o).abs().max()


@pytest.mark.parametrize("lowres,prompt", [(False, False), (True, False), (True, True)], ids=["base", "lowres", "lowres+prompt"])
def test_unet3d_forward_with_cond_images(lowres, prompt, ref_unet3d):
    """Unet3D(cond_images_channels=...) (iv.py:1307-1310, 1722-1731) of the reference vs the oracle: one conditioning image per sample,
    repeated over the frames (also the prompt frames'), resized, concatenated in front of the input channels."""
    from oracle import unet3d_oracle as u3

    kw, ours, x, t, te, extra = rc.unet3d_cond_images_case(lowres, prompt)
    sd = ours.state_dict()
    with torch.no_grad():
        for cdp, r in zip((0.0, 1.0), ref_unet3d[f"cond_images/{lowres}-{prompt}"]):
            o = u3.unet3d_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=cdp, **extra)
            assert r.shape == x.shape and torch.allclose(r, o, atol=1e-4, rtol=1e-4), (r - o).abs().max()
    assert rc.layout(ours) == ref_unet3d[f"cond_images_layout/{lowres}-{prompt}"]


@pytest.mark.parametrize("name", list(__import__("unet_config_sweep").SWEEP))
def test_unet_oracle_config_sweep(name, ref_unet):
    """The oracle against the reference over constructor-flag combinations beyond the README unets (the planner is then checked
    against the oracle for the same configurations in tests/test_plan_interp.py)."""
    kw, u, x, t, te, extra = rc.sweep_case(name)
    assert rc.layout(u) == ref_unet[f"sweep_layout/{name}"], "state_dict layout"
    sd = u.state_dict()
    with torch.no_grad():
        for cdp, r in zip((0.0, 1.0), ref_unet[f"sweep/{name}"]):
            o = uo.unet_forward(sd, kw, x, t, text_embeds=te, cond_drop_prob=cdp, **extra)
            assert r.abs().mean() > 1e-3
            assert torch.allclose(r, o, atol=2e-5, rtol=1e-4), (name, cdp, (r - o).abs().max())


def test_scheduler_tensor_api_is_bit_identical(ref_sampler):
    """GaussianDiffusionContinuousTimes' tensor methods (ip.py:223-318) against the reference's class: same fp32 expressions, same bits."""
    from imagen_pytorch_amd.schedules import GaussianDiffusionContinuousTimes as Ours

    calls = rc.schedule_inputs()
    for ns in ("linear", "cosine"):
        a = Ours(noise_schedule=ns, timesteps=37)
        for name, (method, args, kw) in calls.items():
            ra, rb = getattr(a, method)(*args, **kw), ref_sampler[f"schedule/{ns}/{name}"]
            ra = ra if isinstance(ra, tuple) else (ra,)
            assert len(ra) == len(rb)
            for u, v in zip(ra, rb):
                assert u.shape == v.shape and torch.equal(u, v), (ns, name)
        ta, tb = a.get_sampling_timesteps(4, device="cpu"), ref_sampler[f"schedule/{ns}/timesteps"]
        assert len(ta) == len(tb)
        for (x, y), pq in zip(ta, tb):
            assert torch.equal(x, pq[0]) and torch.equal(y, pq[1])
        assert tuple(a.sample_random_times(5, device="cpu").shape) == ref_sampler[f"schedule/{ns}/random_times_shape"]


@pytest.mark.parametrize("objective", ["noise", "x_start", "v"])
@pytest.mark.parametrize("dyn", [True, False])
def test_step_level_posterior_math(objective, dyn, ref_sampler):
    """Imagen.p_mean_variance / p_sample around a given model output (no denoiser call): identical to the reference."""
    from imagen_pytorch_amd import Imagen, Unet

    ours = Imagen((Unet(**rc.POSTERIOR_UNET),), image_sizes=(16,), timesteps=10, text_embed_dim=768, cond_drop_prob=0.1)
    x, out, t, tn = rc.posterior_inputs()
    (m2, v2, l2), s2 = ours.p_mean_variance(ours.unets[0], x, t, noise_scheduler=ours.noise_schedulers[0], t_next=tn, model_output=out,
                                            pred_objective=objective, dynamic_threshold=dyn)
    for u, v in zip(ref_sampler[f"posterior/{objective}-{dyn}"], (m2, v2, l2, s2)):
        assert u.shape == v.shape and torch.allclose(u, v, rtol=0, atol=1e-6)


@pytest.mark.parametrize("objective", ["noise", "x_start", "v"])
@pytest.mark.parametrize("dyn", [True, False])
def test_oracle_ddpm_step_posterior_math(objective, dyn, ref_sampler):
    """oracle.ddpm_step on every objective x thresholding (ip.py:2085-2109, 252-270) against the reference's p_mean_variance: with the
    noise term zeroed the step returns the posterior mean, and its x0 is the thresholded x_start."""
    x, out, t, tn = rc.posterior_inputs()
    mean, _, _, x0 = ref_sampler[f"posterior/{objective}-{dyn}"]
    got, got_x0 = so.ddpm_step(x, out, t, tn, torch.zeros_like(x), "cosine", dyn, 0.95, objective)
    assert torch.allclose(got_x0, x0, rtol=0, atol=1e-6), (got_x0 - x0).abs().max()
    assert torch.allclose(got, mean, rtol=0, atol=1e-6), (got - mean).abs().max()
    if dyn:     # the fixture's thresholds do bite: the test could not pass with the static clamp
        assert not torch.allclose(x0, so.predict_x0(x, out, *so.alpha_sigma(so.log_snr_cosine(t).view(-1, 1, 1, 1)), objective).clamp(-1, 1))


def test_cross_embed_downsample_is_unbuildable_in_the_reference(ref_unet):
    """Why `Unet(cross_embed_downsample=True)` stays a NotImplementedError here: the reference's own constructor fails on it
    (`partial(CrossEmbedLayer, kernel_sizes=...)(dim_in, dim_out)`, ip.py:1315 / 1357 / 1366), so no model with that flag exists."""
    from imagen_pytorch_amd import Unet

    assert ref_unet["cross_embed_downsample_error"] == "TypeError"
    with pytest.raises(NotImplementedError):
        Unet(dim=8, dim_mults=(1, 2), cross_embed_downsample=True)
