"""CPU: the conv / GEMM kernels themselves — csrc/igemm.hip, conv_dma.hip, conv_stream.hip — executed by the functional emulation of
tools/emul (a workgroup = cooperative fibers, the wave-level instructions restated from the ISA layouts, direct-to-LDS copies landing at
the covering vmcnt wait in issue order) on 23 cases covering every structural path: tile arrangements, k-loop instantiations, prologues,
both epilogue instantiations with every output mode, partial tiles, several cout tiles, persistent tile walks, the all-DMA pipeline with
GlobalContext partials, the streaming kernel's in-place LDS prologue.

The emulated PRODUCT build has to reproduce the fp32 torch contract (tests/igemm_case.py) at the tolerance the GPU tests use — which
validates the emulator where the kernels are known-good on MI355X, and checks a kernel edit functionally before it costs GPU minutes.
The library is built by __graft_entry__.build() / tools/emul/build_emul_lib.sh (host clang, ~1 min each, cached)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TOL = 1e-3


def _lib(tag=""):
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "emul", "build_emul_lib.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    return os.path.join(ROOT, "imagen-pytorch_amd", "libimagen_emul.so")


def _run(lib, out):
    env = dict(os.environ, IMAGEN_LIB_PATH=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emul", "run_cases.py"), "--out", str(out)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return torch.load(str(out), weights_only=False)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_igemm_matches_contract(tmp_path):
    product = _run(_lib(""), tmp_path / "product.pt")
    assert len(product) >= 39 and sum(n.startswith('pro') for n in product) >= 10
    for name, r in product.items():
        assert r["err"] < TOL, (name, r["err"])
        if "err_ssq" in r:
            assert r["err_ssq"] < 2e-3, (name, r["err_ssq"])
        if "err_gca" in r:
            assert r["err_gca"] < 2e-3, (name, r["err_gca"])


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_channel_slice_outputs():
    """Output stride != Cout (a conv writing its channel slice of a concatenated tensor: the UpsampleCombiner plan) on the emulated product
    kernels: right values, neighbouring channels untouched, wave-specialised and streaming family (tools/emul/run_slice_cases.py)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "emul", "run_slice_cases.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and out.count("neighbours untouched: True") == 6, out[-2000:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_whole_library_runs_gpu_tests():
    """The emulation covers the whole library (capi.hip with recorded graph capture, attention, elementwise, sampler): a slice of the
    `-m gpu` tests — sampler kernels, hipGraph capture / replay, the quantile, the combine_upsample_fmaps forwards — runs on it in a child pytest (IMAGEN_EMUL_TESTS=1, tests/conftest.py)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""), IMAGEN_EMUL_TESTS="1")
    sel = ("test_conv_pro_family or test_conv_gemm_family or graph_capture_replay or ddpm_step_vs_formula or ddpm_step_row_keys or lincomb_masked or quantile_exact or time_embed_scale_shift "
           "or upsample_combiner or test_act_prep or clamp_the_step or temporal_attention_kernel or temporal_peg or (test_global_context and 1024) "
           "or 512-103-True-extreme-False-64 or 512-103-True-extreme-True-64 or linear_f32 or null_value_is_not_rounded")   # round 4: the GEMM family, the MFMA temporal attention, the two-phase GlobalContext finalisation, the bounded-logit attention
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_kernels_gpu.py"), os.path.join(ROOT, "tests", "test_model_gpu.py"),
                        os.path.join(ROOT, "tests", "test_igemm_cfgs_gpu.py"), os.path.join(ROOT, "tests", "test_video_gpu.py"),
                        "-q", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode()
    assert r.returncode == 0 and " passed" in out and "failed" not in out and "skipped" not in out.splitlines()[-1], out[-3000:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_rowchain_kernels():
    """Round 5: csrc/rowchain.hip — the four chains, 32- and 64-row tiles, the K-split layers — on the emulation in a child pytest, against
    the launch-per-op plans they replace and fp32 torch (tests/test_rowchain_gpu.py; the benchmark-sized cases are hardware-only)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_rowchain_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out, out[-3000:]
    passed = int(out.split(" passed")[0].split()[-1])
    assert passed >= 24, out[-800:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_rowchain_contract():
    """csrc/rowchain.hip per row against the fp64 restatement of its contract and the launch-per-op plans, at the shapes the launcher takes beyond
    the engine's: uneven and clamped K-splits, one tile per image, 1 .. 292 keys, a late row maximum, strided rows, sentinels around every output
    (tests/test_rowchain_contract_gpu.py: the whole file, about a minute on the emulation)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_rowchain_contract_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out, out[-3000:]
    passed = int(out.split(" passed")[0].split()[-1])
    assert passed == 44 and "skipped" not in out.splitlines()[-1], out[-800:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_attention_contract():
    """csrc/attention.hip per element against the fp64 restatement of ATTENTION's contract at a derived bound: the four tilings at 1 .. 449 keys and
    1 .. 513 rows, the engine's self / cross layouts and the shared-head form on strided, guarded operands, fused QNORM, logits at the bound,
    a late maximum in some rows of a wave, the launcher's alignment predicates (tests/test_attention_contract_gpu.py: the whole file, about a
    minute on the emulation; no case is hardware-only)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_attention_contract_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out, out[-3000:]
    passed = int(out.split(" passed")[0].split()[-1])
    assert passed == 127 and "skipped" not in out.splitlines()[-1], out[-800:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_conv_contract():
    """Every conv / GEMM kernel family per pixel against the fp64 restatement of the IGEMM contract and the launch-per-op plan, on strided operands
    in guarded allocations: channel slices, maps smaller than a tile, ragged all-cout epilogues, the shortest persistent tile ranges, the
    alignment predicates of launch_igemm inside and outside, every other predicate of the eight launchers just outside (tests/test_conv_contract_gpu.py:
    the whole file, about two minutes on the emulation, which holds every family: nothing skips)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_conv_contract_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1500)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out, out[-3000:]
    passed = int(out.split(" passed")[0].split()[-1])
    assert passed == 387 and "skipped" not in out.splitlines()[-1], out[-800:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_elementwise_kernels():
    """csrc/elementwise.hip — every glue kernel on every branch an engine call site selects, per row / per element against fp64, sentinels
    around every output, the launchers' refusals — on the emulation in a child pytest (tests/test_elementwise_kernels_gpu.py; the whole file
    takes seconds there; only the ACT_PREP launch above the grid cap is left to hardware)."""
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""), IMAGEN_EMUL_TESTS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_elementwise_kernels_gpu.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and "failed" not in out, out[-3000:]
    passed = int(out.split(" passed")[0].split()[-1])
    assert passed >= 409 and " 1 skipped" in out.splitlines()[-1], out[-800:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="host clang of the ROCm toolchain not present")
def test_emulated_kernels_follow_their_contract_launch_by_launch(tmp_path):
    """tools/op_audit.py on the emulation: every launch of README unet1's plans (a 16 x 16 image, the unconditional row) executed by the kernel
    sources and by the plan interpreter FROM IDENTICAL INPUTS.  Two fp32 computations of one quantity round to the same fp16 value almost
    everywhere, so a kernel that follows its contract sits at ~1e-6 from it; the attention kernels and the cross-attention chains, whose fp16 P
    the contract does not model, at 2-4e-4 (the same figures the tool measures on MI355X: profiles/r05_s_op_audit_readme_unet1_null_row.txt)."""
    import json
    out = tmp_path / "audit.json"
    env = dict(os.environ, IMAGEN_LIB_PATH=_lib(""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "op_audit.py"), "--config", "u1", "--size", "16", "--null", "--emul", "--threads", "4",
                        "--json", str(out)], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    rows = json.load(open(out))["rows"]
    fl = [x for x in rows if x["dtype"] == "float16"]
    assert len({(x["plan"], x["idx"]) for x in rows}) >= 200 and len(fl) >= 200
    worst = max(fl, key=lambda x: x["err"])
    assert worst["err"] < 6e-4 and not any(x["nan"] for x in rows), worst
    # (a 4^2 / 2^2 map is a few hundred values: one differently rounded element is 1e-4 of the norm, two or three of them 2e-4 — round 6: a conv
    # of the 2^2 level at 2.1e-4 once the chains in front of it changed its input; such maps get 3e-4)
    loose = [x for x in fl if x["err"] > (2e-4 if x["elems"] >= 4096 else 3e-4)]
    assert all(x["kind"] == "ATTENTION" for x in loose), [(x["kind"], x["label"], x["err"], x["elems"]) for x in loose]
    chains = [x for x in fl if x["kind"] == "ROWCHAIN"]      # round 6: P as fp16 hi + lo pairs — the cross-attention chains follow their contract too
    assert chains and max(x["err"] for x in chains) < 2e-4, max(chains, key=lambda x: x["err"])
    errs = sorted(x["err"] for x in fl)
    assert errs[len(errs) // 2] < 1e-5
