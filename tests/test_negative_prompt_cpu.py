"""CPU: negative prompts — a second text prompt on the null rows of classifier-free guidance (`negative_texts`, `negative_text_embeds`,
`negative_text_masks` on Imagen.sample, ElucidatedImagen.sample, Unet(3D).forward_with_cond_scale, prepare_conditioning, sample_pipelined,
sample_requests and distributed.sample_sharded).  With one, every guided evaluation is neg + (pos - neg) * cond_scale, both at
cond_drop_prob = 0: the reference's forward_with_cond_scale (ip.py:1510-1522) with its second forward given a prompt.

  * host logic on dry engines: broadcast, padding, mask derivation, cropping, the staging rows; every refusal, raised before anything is
    launched; the Conditioning handle; merged requests (src_idx / keep_u8); sample_sharded's slicing; one engine per (rows, size);
  * the planner: forwards (a) prompt 5 / negative 7 tokens and (b) 7 / 3 of tests/golden/negprompt_forward.pt, batch-2 and batch-1
    negatives, on the plan interpreter against the reference's forward of each prompt.  Bar: 1.5 x the larger figure the ordinary pair
    (learned null rows) of the same unet and prompt measures against ITS recording in the same test (tests/test_linear_xattn_gpu.py's rule);
  * the drivers: Imagen.sample 16 -> 32, ElucidatedImagen.sample, a video DDPM run (tests/golden/negprompt_runs.pt) replayed against the
    reference under the bars of tests/test_sample_cpu_replay.py for such runs without a negative prompt — 2e-2 (DDPM cascade, video DDPM),
    3e-2 (Karras) — and each >= 10 bars from its twin recorded without the negative prompt;
  * no regression: without a negative prompt the launch lists of all fixture stages equal those recorded from the parent commit
    (tests/golden/negprompt_parent_launch_list_abi15.json).

Measured here (interpreter): forwards (a) ordinary pair cond 1.14e-3 / null 1.21e-3 (bar 1.81e-3), with a batch-2 negative cond 1.14e-3 /
negative rows 1.10e-3, batch-1 negative rows 1.20e-3; (b) ordinary pair 1.17e-3 / 1.21e-3 (bar 1.81e-3), negative rows 1.16e-3 (batch 2) /
1.36e-3 (batch 1); the guided forward 3.1e-3 (ordinary 2.7e-3).  Replays, stage 1 / stage 2 alone: DDPM 2.3e-3 / 6.6e-4, Karras 1.4e-2 /
1.0e-2, video DDPM 1.5e-3; each 0.33 - 0.46 from its twin without the negative prompt.

On the commit before this feature the tests of sections 1 - 5 that pass a `negative_*` keyword fail with `TypeError: ... unexpected keyword
argument` (test_engine_stages_negative_rows, test_engine_refusals, test_refusals_come_before_any_launch,
test_conditioning_handle_carries_the_negative_prompt, test_merged_requests_with_and_without_a_negative_prompt,
test_pipelined_batches_take_negative_prompts, test_pipelined_cascade_with_an_unguided_stage,
test_pipelined_refusals_come_before_any_thread, test_sample_sharded_slices_the_negative_prompt, both planner tests and the three driver
replays); the fixture and launch-list tests pass on both."""
import functools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fixtures_negprompt as npf  # noqa: E402
from fixtures_negprompt import nerr  # noqa: E402
from plan_interp import run_engine  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401  (the fixture that sends Plan.run / Graph to the interpreter)

BARS = {"ddpm": 2e-2, "edm": 3e-2, "video": 2e-2}


@pytest.fixture()
def no_launch(cpu_backend, monkeypatch):
    """cpu_backend in which running any plan is an error: what is refused must be refused before the first launch."""
    from imagen_pytorch_amd import ops

    def launched(self, stream=None):
        raise AssertionError(f"plan '{self.name}' was launched")
    monkeypatch.setattr(ops.Plan, "run", launched)


def _dry(monkeypatch):
    from imagen_pytorch_amd import engine, engine3d

    monkeypatch.setattr(engine, "UnetEngine", functools.partial(engine.UnetEngine, dry=True))
    monkeypatch.setattr(engine3d, "UnetEngine3D", functools.partial(engine3d.UnetEngine3D, dry=True))


def _dry_engine(B=2):
    from imagen_pytorch_amd.engine import UnetEngine

    return UnetEngine(npf.base_unet(), 2 * B, B, 16, "cpu", dry=True)


KEEP = torch.tensor([True, True, False, False])


# ------------------------------------------------------------------------------------------------ 1. engine staging

def test_engine_stages_negative_rows():
    """te16 / mask_u8 hold 2 * src_batch source rows; the null rows point at the second set with keep = 1; the shorter prompt is
    zero-padded and masked; a batch-1 negative is repeated; a missing mask is any(embeds != 0, -1); both are cropped at max_text_len."""
    eng = _dry_engine()
    g = torch.Generator().manual_seed(3)
    te, neg = torch.randn(2, 5, 32, generator=g), torch.randn(2, 7, 32, generator=g)
    neg[1, 5:] = 0.                                          # sample 1's negative has 5 real tokens: the derived mask must say so
    tm = torch.ones(2, 5, dtype=torch.bool)
    tm[1, 3:] = False
    eng.set_conditioning(text_embeds=te, text_mask=tm, keep=KEEP, lowres_noise_times=None, negative_text_embeds=neg)
    plan, te16, mask_u8, neg_plan = eng._static_plans[7]      # keyed by the longer token count
    assert list(eng._static_plans) == [7] and eng._last_static == [neg_plan, plan]
    assert tuple(te16.shape) == (4, 7, 32) and tuple(mask_u8.shape) == (4, 16)
    assert eng.src_idx.tolist() == [0, 1, 2, 3] and eng.keep_u8.tolist() == [1, 1, 1, 1]
    assert torch.equal(te16[:2, :5], te.half()) and not te16[:2, 5:].any()
    assert torch.equal(te16[2:], neg.half())
    assert mask_u8[0].tolist() == [1] * 5 + [0] * 11 and mask_u8[1].tolist() == [1] * 3 + [0] * 13
    assert mask_u8[2].tolist() == [1] * 7 + [0] * 9 and mask_u8[3].tolist() == [1] * 5 + [0] * 11
    assert [l for _, _, l in neg_plan.ops] == ["text_to_cond(negative)"]
    # a prompt WITHOUT a mask, shorter than the negative: its padding is masked, its own tokens are not
    eng.set_conditioning(text_embeds=te, text_mask=None, keep=KEEP, lowres_noise_times=None, negative_text_embeds=neg)
    assert mask_u8[0].tolist() == [1] * 5 + [0] * 11
    # batch-1 negative, shorter than the prompt, with its mask: repeated over the batch, padded and masked
    nm = torch.tensor([[True, True, False]])
    eng.set_conditioning(text_embeds=neg, text_mask=None, keep=KEEP, lowres_noise_times=None, negative_text_embeds=te[:1, :3],
                         negative_text_mask=nm)
    assert list(eng._static_plans) == [7], "the static plan stays keyed by the token count"
    assert torch.equal(te16[2, :3], te[0, :3].half()) and torch.equal(te16[3], te16[2]) and not te16[2:, 3:].any()
    assert mask_u8[2].tolist() == [1, 1] + [0] * 14 and mask_u8[3].tolist() == mask_u8[2].tolist()
    assert mask_u8[0].tolist() == [1] * 16, "an unpadded prompt without a mask keeps the all-ones mask (ip.py:1619-1632)"
    # without a negative prompt afterwards: the rows are as they always were
    eng.set_conditioning(text_embeds=neg, text_mask=None, keep=KEEP, lowres_noise_times=None)
    assert eng.src_idx.tolist() == [0, 1, 0, 1] and eng.keep_u8.tolist() == [1, 1, 0, 0] and eng._last_static == [plan]
    # cropping at max_text_len (16)
    long_neg = torch.randn(1, 20, 32, generator=g)
    eng.set_conditioning(text_embeds=te, text_mask=tm, keep=KEEP, lowres_noise_times=None, negative_text_embeds=long_neg)
    _, te16, mask_u8, _ = eng._static_plans[16]
    assert torch.equal(te16[2], long_neg[0, :16].half()) and mask_u8[3].tolist() == [1] * 16
    # merged rows: sample 0 without a negative keeps the learned null row
    eng.set_conditioning(text_embeds=te, text_mask=tm, keep=KEEP, lowres_noise_times=None, negative_text_embeds=neg,
                         negative_rows=torch.tensor([False, True]))
    assert eng.src_idx.tolist() == [0, 1, 0, 3] and eng.keep_u8.tolist() == [1, 1, 0, 1]


def test_engine_refusals():
    from imagen_pytorch_amd.engine import UnetEngine

    eng = _dry_engine()
    te = torch.randn(2, 5, 32)
    base = dict(text_embeds=te, text_mask=None, keep=KEEP, lowres_noise_times=None)
    with pytest.raises(AssertionError, match="negative_text_embeds"):
        eng.set_conditioning(**base, negative_text_embeds=torch.randn(3, 4, 32))
    with pytest.raises(AssertionError, match="negative_text_embeds"):
        eng.set_conditioning(**base, negative_text_embeds=torch.randn(2, 4, 24))
    plain = UnetEngine(npf.base_unet(), 2, 2, 16, "cpu", dry=True)        # no null rows
    with pytest.raises(AssertionError, match="negative_text_embeds"):
        plain.set_conditioning(text_embeds=te, text_mask=None, keep=torch.ones(2, dtype=torch.bool), lowres_noise_times=None,
                               negative_text_embeds=te)


# ------------------------------------------------------------------------------------------------ 2. refusals of the public interface

def test_refusals_come_before_any_launch(no_launch):
    from imagen_pytorch_amd import Imagen, Unet

    g = npf.runs_fixture()
    te, neg = g["text_embeds"], g["runs"]["ddpm"]["negative_text_embeds"]
    model = npf.image_model("ddpm")
    kw = dict(text_embeds=te, use_tqdm=False, device="cpu")
    with pytest.raises(ValueError, match="negative_text_embeds.*cond_scale is 1"):
        model.sample(**kw, negative_text_embeds=neg)
    with pytest.raises(ValueError, match="negative_texts.*cond_scale is 1"):
        model.encode_text = lambda texts, return_attn_mask=True: (neg, torch.ones(1, 6, dtype=torch.bool))
        model.sample(**kw, negative_texts=["blurry"], cond_scale=(1., 1.))
    with pytest.raises(ValueError, match="cond_scale is 1"):                      # the stage that runs is unguided, the other does not run
        model.sample(**kw, negative_text_embeds=neg, cond_scale=(1., 3.), stop_at_unet_number=1)
    with pytest.raises(ValueError, match="negative_texts and negative_text_embeds"):
        model.sample(**kw, cond_scale=3., negative_text_embeds=neg, negative_texts=["blurry"])
    with pytest.raises(ValueError, match="negative_text_embeds.*embedding"):
        model.sample(**kw, cond_scale=3., negative_text_embeds=neg[..., :24])
    with pytest.raises(ValueError, match="negative_text_embeds.*batch 3"):
        model.sample(**kw, cond_scale=3., negative_text_embeds=neg.expand(3, -1, -1))
    with pytest.raises(ValueError, match="negative_text_masks"):
        model.sample(**kw, cond_scale=3., negative_text_masks=torch.ones(1, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="negative_text_masks"):
        model.sample(**kw, cond_scale=3., negative_text_embeds=neg, negative_text_masks=torch.ones(1, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="negative_text_embeds.*conditioning"):
        model.sample(conditioning=model.prepare_conditioning(text_embeds=te), cond_scale=3., negative_text_embeds=neg, use_tqdm=False, device="cpu")
    with pytest.raises(ValueError, match="negative_text_embeds.*batch 3"):
        model.prepare_conditioning(text_embeds=te, negative_text_embeds=neg.expand(3, -1, -1))
    with pytest.raises(ValueError, match="negative_text_embeds.*batch 3"):
        model.sample_requests([dict(text_embeds=te, negative_text_embeds=neg.expand(3, -1, -1))], cond_scale=3., device="cpu")
    with pytest.raises(ValueError, match="per request or as a common keyword"):
        model.sample_requests([dict(text_embeds=te, negative_text_embeds=neg)], cond_scale=3., device="cpu", negative_text_embeds=neg)
    # a model that cannot do guidance; a model without text conditioning
    unguided = Imagen((Unet(**npf.base_kwargs()),), image_sizes=(16,), timesteps=2, text_embed_dim=32, cond_drop_prob=0.).eval()
    with pytest.raises(ValueError, match="negative_text_embeds.*conditional dropout"):
        unguided.sample(**kw, negative_text_embeds=neg)
    uncond = Imagen((Unet(**npf.base_kwargs()),), image_sizes=(16,), timesteps=2, condition_on_text=False, cond_drop_prob=0.1).eval()
    with pytest.raises(ValueError, match="negative_text_embeds.*condition_on_text=False"):
        uncond.sample(batch_size=2, cond_scale=3., negative_text_embeds=neg, use_tqdm=False, device="cpu")
    with pytest.raises(ValueError, match="negative_texts.*condition_on_text=False"):
        uncond.prepare_conditioning(batch_size=2, negative_texts=["blurry"])
    # the unets' own guided forward
    f = npf.forward_fixture()
    c = f["cases"]["a"]
    u = npf.base_unet()
    tk = dict(text_embeds=c["text_embeds"], text_mask=c["text_mask"])
    for bad, frag in ((dict(negative_text_embeds=c["negative_text_embeds"][..., :24]), "negative_text_embeds: invalid text embedding shape"),
                      (dict(negative_text_embeds=c["negative_text_embeds"][:1].expand(3, -1, -1)), "negative_text_embeds: batch 3"),
                      (dict(negative_texts=["blurry"]), "negative_texts"),
                      (dict(negative_text_masks=c["negative_text_mask"]), "negative_text_masks"),
                      (dict(negative_text_embeds=c["negative_text_embeds"], negative_text_masks=c["negative_text_mask"][:, :2]), "negative_text_masks")):
        with pytest.raises(ValueError, match=frag):
            u.forward_with_cond_scale(f["x"], f["time"], cond_scale=3., **tk, **bad)
    with pytest.raises(ValueError, match="negative_text_embeds: cond_scale is 1"):
        u.forward_with_cond_scale(f["x"], f["time"], **tk, negative_text_embeds=c["negative_text_embeds"])
    with pytest.raises(ValueError, match="negative_text_embeds.*not conditioned on text"):
        u.forward_with_cond_scale(f["x"], f["time"], cond_scale=3., negative_text_embeds=c["negative_text_embeds"])
    from imagen_pytorch_amd import Unet3D
    v = Unet3D(**npf.video_kwargs()).eval()
    with pytest.raises(ValueError, match="negative_text_embeds: batch 3"):
        v.forward_with_cond_scale(torch.zeros(2, 3, 4, 16, 16), f["time"], cond_scale=3., text_embeds=c["text_embeds"],
                                  negative_text_embeds=c["negative_text_embeds"][:1].expand(3, -1, -1))


# ------------------------------------------------------------------------------------------------ 3. handle, requests, pipeline, shards

def _stub_stages(monkeypatch, klass=None):
    """Dry engines and a stage loop that returns zeros: sample() runs all of its host logic and launches nothing."""
    from imagen_pytorch_amd import Imagen, ops

    _dry(monkeypatch)
    monkeypatch.setattr(klass or Imagen, "_run_stage", lambda self, st, **kw: torch.zeros_like(st["eng"].x_in))
    monkeypatch.setattr(ops.Plan, "run", lambda self, stream=None: None)       # (the low-res preparation of stage 2)


def _staged(eng, n_tok):
    _, te16, mask_u8, _ = eng._static_plans[n_tok]
    return te16.clone(), mask_u8.clone(), eng.src_idx.clone(), eng.keep_u8.clone()


def test_conditioning_handle_carries_the_negative_prompt(cpu_backend, monkeypatch):
    _stub_stages(monkeypatch)
    g = npf.runs_fixture()
    te, neg = g["text_embeds"], g["runs"]["video"]["negative_text_embeds"]
    nm = torch.ones(2, 11, dtype=torch.bool)
    nm[0, 8:] = False
    model = npf.image_model("ddpm")
    model.sample(text_embeds=te, cond_scale=3., negative_text_embeds=neg, negative_text_masks=nm, use_tqdm=False, device="cpu")
    engs = [st["eng"] for st in model._stages.values()]
    want = [_staged(e, 11) for e in engs]
    assert all(w[2].tolist() == [0, 1, 2, 3] and w[3].tolist() == [1, 1, 1, 1] for w in want)
    handle = model.prepare_conditioning(text_embeds=te, negative_text_embeds=neg, negative_text_masks=nm)
    assert torch.equal(handle.negative_text_embeds, neg) and torch.equal(handle.negative_text_masks, nm)
    model.sample(text_embeds=te * 2, cond_scale=3., use_tqdm=False, device="cpu")                    # something else in between
    assert engs[0].keep_u8.tolist() == [1, 1, 0, 0] and engs[0].src_idx.tolist() == [0, 1, 0, 1]
    model.sample(conditioning=handle, cond_scale=3., use_tqdm=False, device="cpu")
    got = [_staged(e, 11) for e in engs]
    assert all(all(torch.equal(a, b) for a, b in zip(w, h)) for w, h in zip(want, got))
    runs = [e.static_runs for e in engs]
    model.sample(conditioning=handle, cond_scale=3., use_tqdm=False, device="cpu")                    # the reuse path: the static plan is skipped
    assert [e.static_runs for e in engs] == runs
    # negative_texts goes through the same encode_text hook as texts
    seen = []

    def hook(texts, return_attn_mask=True):
        seen.append(list(texts))
        return neg[:len(texts)], nm[:len(texts)]
    model.encode_text = hook
    h2 = model.prepare_conditioning(text_embeds=te, negative_texts=["blurry"])
    assert seen == [["blurry"]] and tuple(h2.negative_text_embeds.shape) == (1, 11, 32)
    model.sample(text_embeds=te, cond_scale=3., negative_texts=["low quality", "blurry"], use_tqdm=False, device="cpu")
    assert seen[-1] == ["low quality", "blurry"]
    assert all(all(torch.equal(a, b) for a, b in zip(w, _staged(e, 11))) for w, e in zip(want, engs))
    # one engine per (rows, size), with and without a negative prompt: the two stages, nothing else
    assert len(model._stages) == 2 and [st["eng"] for st in model._stages.values()] == engs
    assert sorted((e.R, e.S) for e in engs) == [(4, 16), (4, 32)]


def test_merged_requests_with_and_without_a_negative_prompt(cpu_backend, monkeypatch):
    _stub_stages(monkeypatch)
    g = npf.runs_fixture()
    te, neg = g["text_embeds"], g["runs"]["ddpm"]["negative_text_embeds"]          # neg: (1, 6, 32)
    model = npf.image_model("ddpm")
    reqs = [dict(text_embeds=te[:, :7], seed=1), dict(text_embeds=te[:1], negative_text_embeds=neg, seed=2),
            dict(text_embeds=te, negative_text_embeds=neg.expand(2, -1, -1)[:, :4], negative_text_masks=torch.tensor([[True] * 4, [True] * 3 + [False]]), seed=3)]
    outs = model.sample_requests(reqs, cond_scale=3., device="cpu")
    assert [o.shape[0] for o in outs] == [2, 1, 2]
    for st in model._stages.values():
        eng = st["eng"]
        assert eng.R == 10
        te16, mask_u8, src_idx, keep_u8 = _staged(eng, 9)
        assert src_idx.tolist() == [0, 1, 2, 3, 4, 0, 1, 7, 8, 9], "null rows of the first request stay on the prompts' rows, unused"
        assert keep_u8.tolist() == [1] * 5 + [0, 0, 1, 1, 1], "… with keep = 0: the learned null conditioning"
        assert torch.equal(te16[7, :6], neg[0].half()) and torch.equal(te16[8, :4], neg[0, :4].half()) and not te16[8, 4:].any()
        assert mask_u8[7].tolist() == [1] * 6 + [0] * 10 and mask_u8[8].tolist() == [1] * 4 + [0] * 12 and mask_u8[9].tolist() == [1] * 3 + [0] * 13
        assert not te16[5:7].any() and not mask_u8[5:7].any()
    # the same requests without any negative prompt afterwards: the same engines, the rows of before this feature
    model.sample_requests([{k: v for k, v in r.items() if not k.startswith("negative")} for r in reqs], cond_scale=3., device="cpu")
    assert len(model._stages) == 2
    for st in model._stages.values():
        assert st["eng"].src_idx.tolist() == [0, 1, 2, 3, 4] * 2 and st["eng"].keep_u8.tolist() == [1] * 5 + [0] * 5
    # a negative prompt common to all requests
    model.sample_requests(reqs[:1] + [dict(text_embeds=te[:1], seed=2)], cond_scale=3., device="cpu", negative_text_embeds=neg)
    eng = [st["eng"] for st in model._stages.values() if st["eng"].R == 6][0]
    assert eng.keep_u8.tolist() == [1] * 6 and eng.src_idx.tolist() == [0, 1, 2, 3, 4, 5]


def test_pipelined_batches_take_negative_prompts(cpu_backend):
    """sample_pipelined: per batch or common, each batch bit-identical to its own sample() call (one stage step each, on the interpreter)."""
    g = npf.runs_fixture()
    run = g["runs"]["ddpm"]
    te, neg = g["text_embeds"], run["negative_text_embeds"]
    model = npf.image_model("ddpm")
    common = dict(cond_scale=3., device="cpu", max_steps=1, noise_fn=lambda t, shape: run["noise"][t])
    batches = [dict(text_embeds=te, negative_text_embeds=neg), dict(text_embeds=te)]
    seq = [model.sample(use_tqdm=False, **common, **b) for b in batches]
    pipe = model.sample_pipelined(batches, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(seq[0], seq[1])
    both = model.sample_pipelined([dict(text_embeds=te)], negative_text_embeds=neg, **common)
    assert torch.equal(both[0], seq[0])


@pytest.mark.parametrize("scales", [(3., 1.), (1., 3.)])
def test_pipelined_cascade_with_an_unguided_stage(cpu_backend, scales):
    """A cascade in which ONE stage runs at cond_scale 1 takes a negative prompt (that stage has no null rows): sample_pipelined, whose
    workers run one stage per sample() call, is bit-identical to sample() there too, and encodes negative_texts once per batch."""
    g = npf.runs_fixture()
    run = g["runs"]["ddpm"]
    te, neg = g["text_embeds"], run["negative_text_embeds"]
    model = npf.image_model("ddpm")
    common = dict(cond_scale=scales, device="cpu", max_steps=1, noise_fn=lambda t, shape: run["noise"][t])
    batches = [dict(text_embeds=te, negative_text_embeds=neg), dict(text_embeds=te)]
    seq = [model.sample(use_tqdm=False, **common, **b) for b in batches]
    pipe = model.sample_pipelined(batches, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)) and not torch.equal(seq[0], seq[1])
    seen = []

    def hook(texts, return_attn_mask=True):
        seen.append(list(texts))
        return neg, torch.ones(1, neg.shape[1], dtype=torch.bool)
    model.encode_text = hook
    texts = model.sample_pipelined([dict(text_embeds=te)], negative_texts=["blurry"], **common)
    assert torch.equal(texts[0], seq[0]) and seen == [["blurry"]]


def test_pipelined_refusals_come_before_any_thread(no_launch, monkeypatch):
    """sample_pipelined checks the negative prompt against the whole cascade's scales, before a worker thread exists."""
    import threading

    def started(self):
        raise AssertionError("a worker thread was started")
    monkeypatch.setattr(threading.Thread, "start", started)
    g = npf.runs_fixture()
    te, neg = g["text_embeds"], g["runs"]["ddpm"]["negative_text_embeds"]
    model = npf.image_model("ddpm")
    with pytest.raises(ValueError, match="negative_text_embeds.*cond_scale is 1 on every stage"):
        model.sample_pipelined([dict(text_embeds=te)], negative_text_embeds=neg, cond_scale=(1., 1.), device="cpu")
    with pytest.raises(ValueError, match="negative_text_embeds.*cond_scale is 1 on every stage"):
        model.sample_pipelined([dict(text_embeds=te), dict(text_embeds=te, negative_text_embeds=neg)], device="cpu")
    with pytest.raises(ValueError, match="negative_text_embeds.*batch 3"):
        model.sample_pipelined([dict(text_embeds=te, negative_text_embeds=neg.expand(3, -1, -1))], cond_scale=(3., 1.), device="cpu")
    with pytest.raises(ValueError, match="negative_texts and negative_text_embeds"):
        model.sample_pipelined([dict(text_embeds=te, negative_texts=["blurry"])], negative_text_embeds=neg, cond_scale=3., device="cpu")


def test_sample_sharded_slices_the_negative_prompt(monkeypatch):
    from imagen_pytorch_amd import distributed as d

    te, neg, nm = torch.randn(5, 4, 8), torch.randn(5, 3, 8), torch.rand(5, 3) > 0.3
    calls = []

    def fn(**kw):
        calls.append(kw)
        return torch.zeros(kw["text_embeds"].shape[0], 1)
    d.sample_sharded(fn, te)                                                   # not initialised: one call, no new keyword
    assert set(calls[-1]) == {"text_embeds", "text_masks", "sample_offset"}
    d.sample_sharded(fn, te, negative_text_embeds=neg, negative_text_masks=nm)
    assert torch.equal(calls[-1]["negative_text_embeds"], neg) and torch.equal(calls[-1]["negative_text_masks"], nm)
    monkeypatch.setattr(d.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(d.dist, "get_world_size", lambda group=None: 2)
    for rank, (lo, hi) in enumerate(((0, 3), (3, 5))):
        monkeypatch.setattr(d.dist, "get_rank", lambda group=None, r=rank: r)
        d.sample_sharded(fn, te, negative_text_embeds=neg, negative_text_masks=nm, gather=False)
        kw = calls[-1]
        assert kw["sample_offset"] == lo and torch.equal(kw["text_embeds"], te[lo:hi])
        assert torch.equal(kw["negative_text_embeds"], neg[lo:hi]) and torch.equal(kw["negative_text_masks"], nm[lo:hi])
        d.sample_sharded(fn, te, negative_text_embeds=neg[:1], gather=False)          # batch 1: every rank gets it whole
        assert torch.equal(calls[-1]["negative_text_embeds"], neg[:1]) and calls[-1]["negative_text_masks"] is None
        d.sample_sharded(fn, te, negative_texts=list("abcde"), gather=False)
        assert calls[-1]["negative_texts"] == list("abcde")[lo:hi]
        d.sample_sharded(fn, te, negative_texts=["x"], gather=False)
        assert calls[-1]["negative_texts"] == ["x"]
    with pytest.raises(ValueError, match="negative_text_embeds: batch 2"):
        d.sample_sharded(fn, te, negative_text_embeds=neg[:2], gather=False)
    with pytest.raises(ValueError, match="negative_texts"):
        d.sample_sharded(fn, te, negative_texts=["a", "b"], gather=False)


# ------------------------------------------------------------------------------------------------ 4. planner

def run_pair(u, f, **neg):
    """One guided pair (cond rows, then null rows) of `u` on the inputs f, the null rows on the learned null conditioning or, with `neg`
    (negative_text_embeds, negative_text_mask), on that prompt: (out_cond, out_null, engine)."""
    from imagen_pytorch_amd.engine import UnetEngine

    B, S = f["x"].shape[0], f["x"].shape[-1]
    return run_engine(UnetEngine(u, 2 * B, B, S, "cpu", dry=True), f["x"], f["time"], f["text_embeds"], f["text_mask"], **neg)[:3]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_negative_prompt_plan_on_cpu_matches_reference_forwards(tag):
    from imagen_pytorch_amd import ops

    ops.KEEP_REFERENCE_WEIGHTS = True
    try:
        f = npf.forward_fixture()
        c = f["cases"][tag]
        inp = dict(x=f["x"], time=f["time"], text_embeds=c["text_embeds"], text_mask=c["text_mask"])
        u = npf.base_unet()
        oc, on, _ = run_pair(u, inp)
        o_c, o_n = nerr(oc, c["out_cond"]), nerr(on, c["out_null"])
        guided = nerr(on + (oc - on) * f["cond_scale"], c["out_cfg"])
        bar = 1.5 * max(o_c, o_n)
        pc, pn, eng = run_pair(u, inp, negative_text_embeds=c["negative_text_embeds"], negative_text_mask=c["negative_text_mask"])
        e_c, e_n = nerr(pc, c["out_cond"]), nerr(pn, c["out_neg"])
        qc, qn, _ = run_pair(u, inp, negative_text_embeds=c["negative_text_embeds"][:1], negative_text_mask=c["negative_text_mask"][:1])
        e1_c, e1_n = nerr(qc, c["out_cond"]), nerr(qn, c["out_neg_b1"])
        far = min(nerr(pn, c["out_null"]), nerr(qn, c["out_null"]))
        print(f"negative prompt forward ({tag}): ordinary pair cond {o_c:.3e} null {o_n:.3e} (guided {guided:.3e}), bar {bar:.3e}; with a batch-2 negative "
              f"cond {e_c:.3e} negative rows {e_n:.3e}; batch-1 cond {e1_c:.3e} negative rows {e1_n:.3e}; negative rows from the learned-null recording {far:.3e}")
        assert max(e_c, e_n, e1_c, e1_n) < bar, (e_c, e_n, e1_c, e1_n, bar)
        assert far > 10 * 1e-2, far
        assert torch.equal(qn[0], pn[0]), "sample 0 meets the same negative prompt in both runs"
        n_tok = max(c["text_embeds"].shape[1], c["negative_text_embeds"].shape[1])
        assert list(eng._static_plans) == [n_tok]
    finally:
        ops.KEEP_REFERENCE_WEIGHTS = False
        ops.REFERENCE_WEIGHTS.clear()


def test_unet_guided_forward_and_engine_cache(cpu_backend):
    """Unet.forward_with_cond_scale with the keywords: the combination of the two recorded forwards; the unet keeps ONE engine for the
    guided shape, with or without a negative prompt, and the ordinary call after it is the ordinary call before it, bit for bit."""
    f = npf.forward_fixture()
    c = f["cases"]["a"]
    u = npf.base_unet()
    tk = dict(text_embeds=c["text_embeds"], text_mask=c["text_mask"], cond_scale=f["cond_scale"])
    before = u.forward_with_cond_scale(f["x"], f["time"], **tk)
    out = u.forward_with_cond_scale(f["x"], f["time"], **tk, negative_text_embeds=c["negative_text_embeds"], negative_text_masks=c["negative_text_mask"])
    want = c["out_neg"] + (c["out_cond"] - c["out_neg"]) * f["cond_scale"]
    e, e_ord = nerr(out, want), nerr(before, c["out_cfg"])
    print(f"Unet.forward_with_cond_scale with a negative prompt: {e:.3e} (ordinary guided forward {e_ord:.3e})")
    assert e < 1.5 * e_ord and nerr(out, c["out_cfg"]) > 10 * 1e-2
    assert torch.equal(u.forward_with_cond_scale(f["x"], f["time"], **tk), before)
    # no text_mask, the prompt (5 tokens) shorter than the negative (7): what the docstring says, the call with an all-ones mask over the
    # prompt's own tokens
    nk = dict(negative_text_embeds=c["negative_text_embeds"], negative_text_masks=c["negative_text_mask"])
    te = c["text_embeds"]
    no_mask = u.forward_with_cond_scale(f["x"], f["time"], text_embeds=te, cond_scale=f["cond_scale"], **nk)
    ones = u.forward_with_cond_scale(f["x"], f["time"], text_embeds=te, text_mask=torch.ones(te.shape[:2], dtype=torch.bool), cond_scale=f["cond_scale"], **nk)
    assert te.shape[1] < c["negative_text_embeds"].shape[1] and torch.equal(no_mask, ones)
    assert len(u._engines) == 1


# ------------------------------------------------------------------------------------------------ 5. drivers

def _replay(kind, model, g, extra):
    run = g["runs"][kind]
    nf = lambda t, shape: run["noise"][t]
    common = dict(text_embeds=g["text_embeds"], cond_scale=g["cond_scale"], use_tqdm=False, noise_fn=nf, device="cpu", **extra)
    neg = dict(negative_text_embeds=run["negative_text_embeds"])
    return run, common, neg


@pytest.mark.parametrize("kind", ["ddpm", "edm"])
def test_image_sample_driver_with_negative_prompt(cpu_backend, kind):
    """(c) Imagen.sample / (d) ElucidatedImagen.sample, two stages, through the real driver (time table, graph objects) and eager."""
    g = npf.runs_fixture()
    model = npf.image_model(kind)
    run, common, neg = _replay(kind, model, g, {})
    plain_before = model.sample(return_all_unet_outputs=True, **common)
    outs = model.sample(return_all_unet_outputs=True, **common, **neg)
    assert all(torch.equal(a, b) for a, b in zip(outs, model.sample(return_all_unet_outputs=True, use_graph=False, **common, **neg)))
    e0 = nerr(outs[0], run["outputs"][0])
    alone = model.sample(start_at_unet_number=2, start_image_or_video=run["outputs"][0], **common, **neg)
    e1 = nerr(alone, run["outputs"][1])
    p = [nerr(a, b) for a, b in zip(plain_before, run["outputs_without_negative"])]
    far = min(nerr(a, b) for a, b in zip(outs, run["outputs_without_negative"]))
    print(f"negative prompt {kind} replay: stage 1 {e0:.2e}, stage 2 alone {e1:.2e}; without a negative prompt {p[0]:.2e} / chained {p[1]:.2e}; "
          f"from the twin without one {far:.2e}")
    bar = BARS[kind]
    assert run["bar"] == bar and e0 < bar and e1 < bar, (kind, e0, e1)
    assert p[0] < bar and far > 10 * bar
    # the same model without a negative prompt afterwards: bit-identical to before, on the same engines
    assert all(torch.equal(a, b) for a, b in zip(model.sample(return_all_unet_outputs=True, **common), plain_before))
    assert len(model._stages) == 2, "one stage (engine, graphs) per (rows, size), with or without a negative prompt"


def test_video_sample_driver_with_negative_prompt(cpu_backend):
    """(e) a video DDPM run of 4 frames, one negative prompt per sample, longer than the prompts."""
    g = npf.runs_fixture()
    model = npf.video_model()
    run, common, neg = _replay("video", model, g, dict(video_frames=g["frames"]))
    plain_before = model.sample(**common)
    out = model.sample(**common, **neg)
    assert tuple(out.shape) == tuple(run["outputs"][0].shape)
    assert torch.equal(out, model.sample(use_graph=False, **common, **neg))
    e, p, far = nerr(out, run["outputs"][0]), nerr(plain_before, run["outputs_without_negative"][0]), nerr(out, run["outputs_without_negative"][0])
    print(f"negative prompt video DDPM replay: {e:.2e}; without a negative prompt {p:.2e}; from the twin without one {far:.2e}")
    assert run["bar"] == BARS["video"] and e < BARS["video"] and p < BARS["video"] and far > 10 * BARS["video"]
    assert torch.equal(model.sample(**common), plain_before)
    assert len(model._stages) == 1


def test_fixtures_tell_the_negative_prompt_from_its_absence():
    """From the stored tensors alone: every recorded run lies >= 10 bars from its twin recorded without the negative prompt."""
    g = npf.runs_fixture()
    assert g["discrimination"] == 10.0
    for kind, bar in BARS.items():
        run = g["runs"][kind]
        assert run["bar"] == bar
        for a, b in zip(run["outputs_without_negative"], run["outputs"]):
            assert nerr(a, b) >= 10 * bar, (kind, nerr(a, b))
    f = npf.forward_fixture()
    for tag in ("a", "b"):
        c = f["cases"][tag]
        assert min(nerr(c["out_null"], c["out_neg"]), nerr(c["out_null"], c["out_neg_b1"])) >= 10 * 1e-2
    a, b = f["cases"]["a"], f["cases"]["b"]
    assert (a["text_embeds"].shape[1], a["negative_text_embeds"].shape[1]) == (5, 7)
    assert (b["text_embeds"].shape[1], b["negative_text_embeds"].shape[1]) == (7, 3)


# ------------------------------------------------------------------------------------------------ 6. no regression

def test_launch_lists_without_a_negative_prompt_are_the_parent_commits(monkeypatch):
    """Image DDPM, Karras and video fixture stages, no negative prompt: op kinds and labels of the static plan, the engine's step plan and
    the stage's per-step plan(s) equal the lists recorded from the commit before this feature."""
    from imagen_pytorch_amd import _abi

    _dry(monkeypatch)
    assert _abi.ENUMS["IMAGEN_ABI_VERSION"] == 15, "no ABI change: select_rows already takes an index and a keep flag per row"
    want = json.load(open(os.path.join(npf.GOLDEN, "negprompt_parent_launch_list_abi15.json")))
    got = npf.launch_lists()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
