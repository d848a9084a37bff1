"""The explorers of the reference (src/explorers/*.jl, examples/ising.jl) and what each asks of the device engine: `engine_kw(self)`
returns the explorer's keyword arguments of Engine (its EXPLORER_* code and parameters)."""
from dataclasses import dataclass, field
from typing import Any

from . import _lib


def engine_kw(explorer):
    """the Engine keyword arguments of any explorer: None is "no exploration" (TestSwapper), a class without engine_kw is refused"""
    if explorer is None:
        return dict(explorer=_lib.EXPLORER_NONE)
    if not hasattr(explorer, "engine_kw"):
        raise NotImplementedError("explorer %r is not available on the device" % (explorer,))
    return explorer.engine_kw()


@dataclass
class IsingMetropolis:
    """examples/ising.jl:91-93"""
    n_steps: int = 3

    def engine_kw(self): return dict(explorer=_lib.EXPLORER_ISING_METROPOLIS, slice_n_passes=self.n_steps)


@dataclass
class CheckerboardMetropolis:
    """The two-colour (red / black) Metropolis sweep of IsingLogPotential and SpinGlassLogPotential (the project's own
    specification): n_steps sweeps of two half-sweeps each, all sites of a colour decided at once.  base_length must be even."""
    n_steps: int = 3

    def engine_kw(self): return dict(explorer=_lib.EXPLORER_CHECKERBOARD_METROPOLIS, slice_n_passes=self.n_steps)


@dataclass
class SliceSampler:
    """src/explorers/SliceSampler.jl:8-20"""
    w: float = 10.0
    p: int = 20
    n_passes: int = 3
    max_iter: int = 1024

    def engine_kw(self):
        return dict(explorer=_lib.EXPLORER_SLICE, slice_w=self.w, slice_p=self.p, slice_n_passes=self.n_passes,
                    slice_max_iter=self.max_iter)


@dataclass
class ToyExplorer:
    """src/explorers/ToyExplorer.jl:5"""

    def engine_kw(self): return dict(explorer=_lib.EXPLORER_TOY)


@dataclass
class IdentityPreconditioner:
    """src/explorers/Preconditioner.jl:14"""


@dataclass
class DiagonalPreconditioner:
    """src/explorers/Preconditioner.jl:22"""


@dataclass
class MixDiagonalPreconditioner:
    """src/explorers/Preconditioner.jl:43-52 (default proportions 1//3, 1//3)"""
    p0: float = 1.0 / 3.0
    p1: float = 1.0 / 3.0


def _preconditioner_kw(pc):
    """am_preconditioner (0 identity, 1 diagonal, 2 mixed) and the mixing proportions, as AutoMALA, MALA and AAPS pass them"""
    kind = 0 if isinstance(pc, IdentityPreconditioner) else 1 if isinstance(pc, DiagonalPreconditioner) else 2
    return dict(am_preconditioner=kind, am_p0=getattr(pc, "p0", 0.0), am_p1=getattr(pc, "p1", 0.0))


def _langevin_kw(ex, code):
    """AutoMALA and MALA differ on the device in their code only"""
    return dict(explorer=code, am_base_n_refresh=ex.base_n_refresh, am_exponent_n_refresh=ex.exponent_n_refresh,
                am_step_size=ex.step_size, **_preconditioner_kw(ex.preconditioner))


@dataclass
class AutoMALA:
    """src/explorers/AutoMALA.jl:29-68"""
    base_n_refresh: int = 3
    exponent_n_refresh: float = 0.35
    step_size: float = 1.0
    preconditioner: Any = field(default_factory=MixDiagonalPreconditioner)
    estimated_target_std_deviations: Any = None

    def engine_kw(self): return _langevin_kw(self, _lib.EXPLORER_AUTOMALA)


@dataclass
class MALA:
    """src/explorers/MALA.jl:19-61 (the step size is NOT adapted; the preconditioner is)"""
    base_n_refresh: int = 3
    exponent_n_refresh: float = 0.35
    step_size: float = 1.0
    preconditioner: Any = field(default_factory=MixDiagonalPreconditioner)
    estimated_target_std_deviations: Any = None

    def engine_kw(self): return _langevin_kw(self, _lib.EXPLORER_MALA)


@dataclass
class AAPS:
    """src/explorers/AAPS.jl: the apogee-to-apogee path sampler (Sherlock, Urbas & Ludkin, JCGS 2023).  One transition per explore!;
    K segments besides the current one; the step size is NOT adapted, the preconditioner is (as MALA's)."""
    step_size: float = 1.0
    K: int = 5
    preconditioner: Any = field(default_factory=MixDiagonalPreconditioner)
    estimated_target_std_deviations: Any = None

    def engine_kw(self): return dict(explorer=_lib.EXPLORER_AAPS, am_step_size=self.step_size, aaps_K=self.K, **_preconditioner_kw(self.preconditioner))


@dataclass
class Compose:
    """src/explorers/Compose.jl:5-8: deterministic composition, e.g. Compose(SliceSampler(), AutoMALA())"""
    first: Any = None
    second: Any = None

    def engine_kw(self):
        """the first half's arguments, the second's beside them and its code as explorer2; what the device cannot compose is refused"""
        if isinstance(self.first, Compose) or isinstance(self.second, Compose):
            raise NotImplementedError("nested Compose is not available on the device")
        if isinstance(self.first, AAPS) or isinstance(self.second, AAPS):
            raise NotImplementedError("AAPS is not available as half of a Compose on the device")
        k1, k2 = engine_kw(self.first), engine_kw(self.second)
        if any(k1[k] != k2[k] for k in (set(k1) & set(k2)) - {"explorer"}):
            raise NotImplementedError("Compose of two samplers of the same family needs identical parameters on the device")
        explorer2 = k2.pop("explorer")
        return {**k1, **k2, "explorer2": explorer2}
