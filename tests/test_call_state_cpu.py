"""(CPU) No state of a sample() call survives it.  What a call was given and what was resolved from it travels in one record
(imagen._Call) from sample() / sample_requests / the sample_pipelined workers through the stage loop; the model's thread-local state is the
lane index and nothing else.  After a call with a negative prompt, a refused call, merged requests, a pipelined cascade and a Karras call
with sigma overrides, `vars(model._tls)` holds at most `lane`, and a following plain call is bit-equal to the same call on a fresh model."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import fixtures_negprompt as npf  # noqa: E402
from test_sample_cpu_replay import cpu_backend  # noqa: E402,F401  (Plan.run / Graph on the plan interpreter)


def _clean(model):
    return set(vars(model._tls)) <= {"lane"}


@pytest.mark.parametrize("kind", ["ddpm", "edm"])
def test_no_call_state_survives_a_call(cpu_backend, monkeypatch, kind):
    from imagen_pytorch_amd import Imagen

    g = npf.runs_fixture()
    run = g["runs"][kind]
    te, neg = g["text_embeds"], run["negative_text_embeds"]
    kw = dict(cond_scale=3., device="cpu", max_steps=1, noise_fn=lambda t, shape: run["noise"][t])
    model = npf.image_model(kind)
    assert _clean(model)
    with_neg = model.sample(text_embeds=te, negative_text_embeds=neg, use_tqdm=False, **kw)
    assert _clean(model)
    with pytest.raises(ValueError, match="silently ignored"):                     # refused in the resolve part: nothing to clean up
        model.sample(text_embeds=te, negative_text_embeds=neg, use_tqdm=False, **{**kw, "cond_scale": 1.})
    assert _clean(model)
    handle = model.prepare_conditioning(text_embeds=te, negative_text_embeds=neg)
    with pytest.raises(ValueError, match="carries its own negative prompt"):
        model.sample(conditioning=handle, negative_text_embeds=neg, use_tqdm=False, **kw)
    assert _clean(model)
    if kind == "ddpm":
        # merged requests take no noise_fn and the interpreter no in-kernel noise: the host side of the call with the stage loop stubbed
        with monkeypatch.context() as mp:
            mp.setattr(Imagen, "_run_stage", lambda self, st, **k: torch.zeros_like(st["eng"].x_in))
            outs = model.sample_requests([dict(text_embeds=te, seed=1), dict(text_embeds=te[:1], negative_text_embeds=neg[:1], seed=2)],
                                         cond_scale=3., device="cpu")
        assert [o.shape[0] for o in outs] == [2, 1] and _clean(model)
    else:
        model.sample(text_embeds=te, sigma_min=0.01, sigma_max=40., use_tqdm=False, **kw)
        assert _clean(model)
    pipe = model.sample_pipelined([dict(text_embeds=te, negative_text_embeds=neg)], **kw)
    assert _clean(model) and torch.equal(pipe[0], with_neg)
    plain = model.sample(text_embeds=te, use_tqdm=False, **kw)
    assert _clean(model)
    fresh = npf.image_model(kind).sample(text_embeds=te, use_tqdm=False, **kw)
    assert torch.equal(plain, fresh) and not torch.equal(plain, with_neg)
