"""MI355X (-m gpu): tiled sampling of Imagen.sample on the HIP path — T B (2 T B) denoiser rows at the tile's size and TILES (csrc/tiles.hip)
around them.  The kernel itself is checked per element by tests/test_tiles_kernel_gpu.py; here:

  * the recorded runs of the restatement (tests/fixtures_tile.py, tests/golden/tile_runs.pt), bar 2e-2 (the sample bar of
    tests/test_compose_gpu.py and tests/test_solver_gpu.py), every stage >= 10 bars from its untiled twin's; hipGraph replay == eager
    launches and a second call on the cached stages == the first, bit for bit;
  * T = 1 on every stage == the call without the keywords, bit for bit;
  * lanes == sequential, sample_pipelined == own calls, sample_sharded == unsharded, bit-exact."""
import os
import sys
import threading

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures_solver as fs  # noqa: E402
import fixtures_tile as ft  # noqa: E402
from conftest import gpu_device, record_parity  # noqa: E402
from fixtures_tile import nerr  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 2e-2


@pytest.mark.parametrize("name", list(ft.groups()))
def test_recorded_runs_vs_restatement(name):
    dev = gpu_device()
    g = fs.cascade_fixture()
    grp, rec = ft.groups()[name], ft.runs_fixture()["groups"][name]
    steps, want, twin = rec["steps"], rec["run"], ft.twins_fixture()[name]
    model = ft.group_model(grp, dev, steps)
    call = dict(text_embeds=g["text_embeds"].to(dev), cond_scale=ft.COND_SCALE, use_tqdm=False, noise_fn=fs.fixed_noise(ft.noise_fixture(), dev),
                return_all_unet_outputs=True, **ft.keywords(grp, steps, dev))
    outs = [o.cpu() for o in model.sample(**call)]
    errs = [nerr(o, w) for o, w in zip(outs, want)]
    gaps = [nerr(o, t) for o, t in zip(outs, twin)]
    print(f"{name} at {steps} steps vs the restatement: {errs}; from the untiled twin {gaps}")
    record_parity(f"tile_sample[{name}]", **{f"stage{i + 1}": e for i, e in enumerate(errs)}, **{f"gap_stage{i + 1}": e for i, e in enumerate(gaps)})
    assert [tuple(o.shape) for o in outs] == [tuple(w.shape) for w in want]
    assert max(errs) < BAR, errs
    assert min(gaps) > 10 * BAR, gaps
    eager = model.sample(**{**call, "use_graph": False})
    assert all(torch.equal(a, b.cpu()) for a, b in zip(outs, eager)), "graph replay != eager"
    again = model.sample(**call)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(outs, again)), "second sample() on the cached stages differs"


@pytest.mark.parametrize("sampler", ["ddpm", "dpmpp_2m"])
def test_one_tile_is_the_untiled_call(sampler):
    dev = gpu_device()
    g = fs.cascade_fixture()
    model = fs.cascade_model(dev, timesteps=4)
    kw = dict(text_embeds=g["text_embeds"].to(dev), cond_scale=ft.COND_SCALE, use_tqdm=False, seed=21, return_all_unet_outputs=True,
              **({} if sampler == "ddpm" else dict(sampler=sampler, sample_steps=5)))
    a = model.sample(**kw)
    b = model.sample(tile_shapes=((16, 16), 32), tile_overlap=(3, (5, 0)), **kw)
    assert len(model._stages) == 4 and all(torch.equal(x, y) for x, y in zip(a, b)), "T = 1 != the plain call"


def test_lanes_pipelined_and_sharded():
    """Two lanes from two threads == the same calls in turn; sample_pipelined with tile_shapes as a per-batch key == each batch's own call;
    sample_sharded (one process: the whole batch as one shard) == the unsharded call."""
    from imagen_pytorch_amd.distributed import sample_sharded

    dev = gpu_device()
    g = fs.cascade_fixture()
    model = fs.cascade_model(dev)
    te = g["text_embeds"].to(dev)
    common = dict(cond_scale=ft.COND_SCALE, sampler="dpmpp_2m", sample_steps=4, use_tqdm=False, image_shapes=((16, 24), (32, 48)), tile_overlap=((8, 4), 16))
    calls = [dict(text_embeds=te, seed=31, tile_shapes=((16, 16), (32, 32))), dict(text_embeds=te * 0.9, seed=32, tile_shapes=((16, 16), None))]
    seq = [model.sample(**common, **c) for c in calls]
    plain = model.sample(**{k: v for k, v in common.items() if k != "tile_overlap"}, text_embeds=te, seed=31)
    assert nerr(seq[0], plain) > BAR
    got = [None, None]

    def work(i):
        with model.lane(i + 1), torch.cuda.device(dev):
            got[i] = model.sample(**common, **calls[i])
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert all(o is not None and torch.equal(o, s) for o, s in zip(got, seq)), "lanes != sequential"
    pipe = model.sample_pipelined(calls, **common)
    assert all(torch.equal(a, b) for a, b in zip(pipe, seq)), "sample_pipelined != own calls"
    assert torch.equal(sample_sharded(model.sample, te, seed=31, tile_shapes=((16, 16), (32, 32)), **common), seq[0]), "sample_sharded != unsharded"
