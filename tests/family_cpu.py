"""The checks that the CPU tests of the target families share, held once -- the counterpart of tests/family_gpu.py for a machine without a
device: tests/test_glm_cpu.py, _hier, _ar1, _dense, _mixture, _mixture_model, _varsel and _changepoint name their enum values, their header
and Julia fragments, their grids, their refusal tables and their argtypes, and call these.  Wherever those files differ it is an argument
here, and each call site passes its own: nothing in this module names a family, a message or a number of one.

Nothing here builds or imports the package at import: the P fixture does both, when a test first asks for it."""
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "include", "pte.h")) as _f:
    HEADER = _f.read()
with open(os.path.join(ROOT, "pigeons.jl_amd", "julia", "PigeonsMI355X.jl")) as _f:
    JULIA = _f.read()


@pytest.fixture(scope="module")
def P():
    import __graft_entry__ as g
    g.build_hip()
    import pigeons_amd
    return pigeons_amd


def no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")


# ---- pte_create and the setters, as far as a machine without a device gets ---------------------------------------------------------------
def assert_reaches_the_device_check(P, **config):
    """config passes validate_config: what refuses it is the missing device"""
    with pytest.raises(P.PteError, match="no HIP device"):
        P.Engine(**config)


def assert_create_refused(P, base, kw, msg):
    """base with kw over it is refused with msg"""
    args = dict(base)
    args.update(kw)
    with pytest.raises(P.PteError, match=msg):
        P.Engine(**args)


def assert_null_engine_refused(fn, args, argtypes, n_args=None):
    """fn, a bound export of the library: argtypes[i] is the ctypes type of argument i (n_args of them, where given), and fn(*args) with a
    null engine returns 1 -- it is refused, not dereferenced"""
    for i, t in argtypes.items():
        assert fn.argtypes[i] is t, (i, fn.argtypes[i])
    assert n_args is None or len(fn.argtypes) == n_args
    assert fn(*args) == 1


# ---- the Python mapping, on an engine that records ---------------------------------------------------------------------------------------
class RecordingEngine:
    """stands in for pigeons_amd.engine.Engine under PT(engine_factory=...): `kw` holds the constructor's keyword arguments, `calls[name]`
    the positional arguments of every call of a setter `name`, as passed.  A setter that Engine has not, or arguments that Engine's would
    not take, fail here as they would there."""

    def __init__(self, **kw):
        self.kw, self.calls = kw, {}
        self.N, self.d = kw["n_chains"], kw["dim"]

    def __getattr__(self, name):
        from pigeons_amd.engine import Engine
        if not name.startswith("set_"):
            raise AttributeError(name)
        sig = inspect.signature(getattr(Engine, name))

        def record(*args, **kwargs):
            self.calls.setdefault(name, []).append(sig.bind(self, *args, **kwargs).args[1:])
        return record


def captured(P, target, explorer=None, reference="default", ref_dim=None, **kw):
    """PT of four chains over one RecordingEngine (reference: ScaledPrecisionNormal(0.5) of ref_dim, target.dim unless given) -> the
    engine's constructor keywords, and its setter calls under the setters' names"""
    if reference == "default":
        reference = P.ScaledPrecisionNormalLogPotential(0.5, target.dim if ref_dim is None else ref_dim)
    pt = P.PT(P.Inputs(target=target, reference=reference, n_chains=4, n_rounds=2, explorer=explorer, show_report=False, **kw),
              engine_factory=RecordingEngine)
    return {**pt.replicas.kw, **pt.replicas.calls}


def assert_reference_refusals(P, target, wrong_dim, **kw):
    """no reference, a ScaledPrecisionNormal of wrong_dim coordinates and a GaussianReference are each refused (kw: as for captured)"""
    with pytest.raises(NotImplementedError, match="reference=ScaledPrecisionNormalLogPotential"):
        captured(P, target, reference=None, **kw)
    with pytest.raises(NotImplementedError, match="reference=ScaledPrecisionNormalLogPotential"):
        captured(P, target, reference=P.ScaledPrecisionNormalLogPotential(1.0, wrong_dim), **kw)
    with pytest.raises(NotImplementedError, match="GaussianReference"):
        captured(P, target, variational=P.GaussianReference(), **kw)


def assert_every_shard_gets_the_data(P, target, reference, N, d, setter):
    """PT on two shards: two distinct engines of N chains and d coordinates had `setter` called, and they are exactly pt.shards.engines"""
    made = []

    def make(**kw):
        made.append(RecordingEngine(**kw))
        return made[-1]
    pt = P.PT(P.Inputs(target=target, reference=reference, n_chains=N, n_rounds=2, show_report=False), engine_factory=make, n_shards=2)
    seen = [e for e in made if setter in e.calls]
    assert len(seen) == 2 and seen[0] is not seen[1] and set(seen) == set(pt.shards.engines)
    assert all((e.N, e.d) == (N, d) and len(e.calls[setter]) == 1 for e in seen)
