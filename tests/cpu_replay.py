"""The real sampling driver on the CPU: `ops.Plan.run` and `ops.Graph` go to a plan interpreter (tests/plan_interp.py), the few `torch.cuda`
calls of the driver become no-ops, and the device checks admit 'cpu'.  TEST INFRASTRUCTURE, never imported by the product, which has no CPU
path.  A plain context manager: the `cpu_backend` fixture of tests/test_sample_cpu_replay.py and tools/sampler_digests.py both enter it."""
from __future__ import annotations

import contextlib

import torch


class _Stream:
    device = torch.device("cpu")
    cuda_stream = 0

    def __init__(self, *a, **k):
        pass

    def synchronize(self):
        pass

    def wait_stream(self, other):
        pass

    def wait_event(self, ev):
        pass


class _Event:
    def __init__(self, *a, **k):
        pass

    def record(self, stream=None):
        pass


class _Graph:
    def __init__(self, plan, stream):
        self.plan = plan

    def launch(self):
        self.plan.run()


@contextlib.contextmanager
def cpu_backend(interpreter=None):
    """Patch the product for the duration of the block and yield the interpreter (a fresh plan_interp.Interpreter unless one is given)."""
    from imagen_pytorch_amd import imagen as imagen_mod
    from imagen_pytorch_amd import ops
    from imagen_pytorch_amd import unet as unet_mod
    from plan_interp import Interpreter

    it = Interpreter() if interpreter is None else interpreter
    null = lambda *a, **k: contextlib.nullcontext()
    patches = [(ops, "KEEP_REFERENCE_WEIGHTS", True), (ops.Plan, "run", lambda self, stream=None: it.run(self)), (ops, "Graph", _Graph),
               (imagen_mod, "_SAMPLING_DEVICE_TYPES", ("cuda", "cpu")), (unet_mod, "_ENGINE_DEVICE_TYPES", ("cuda", "cpu")),
               (torch.cuda, "Stream", _Stream), (torch.cuda, "Event", _Event), (torch.cuda, "current_stream", lambda *a, **k: _Stream()),
               (torch.cuda, "synchronize", lambda *a, **k: None), (torch.cuda, "device", null), (torch.cuda, "stream", null)]
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in patches]
    for obj, name, value in patches:
        setattr(obj, name, value)
    try:
        yield it
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
        ops.REFERENCE_WEIGHTS.clear()
