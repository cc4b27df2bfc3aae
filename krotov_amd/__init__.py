"""krotov_amd -- MI355X-native Krotov optimal-control engine.

Keeps the plugin surface of qucontrol/krotov (``optimize_pulses`` /
``Objective`` / ``propagator=``) and replaces the per-iteration
backward/forward propagation and pulse-update loop by hand-written CDNA4 HIP
kernels behind a C ABI (include/krotov_hip.h).  See DESIGN.md.
"""
from . import (
    configs,
    constraints,
    convergence,
    conversions,
    functionals,
    info_hooks,
    mu,
    nonlinear,
    objectives,
    parallelization,
    parametrization,
    propagators,
    result,
    second_order,
    shapes,
)
from .objectives import Objective, ensemble_objectives, gate_objectives, propagate_objectives
from .batch import optimize_pulses_batch
from .constraints import QuadraticStateConstraint, StateDependentConstraint
from .gradient import PulseGradient
from .nonlinear import ControlFunction, Power
from .optimize import optimize_pulses
from .parametrization import (
    LinearParametrization,
    Parametrization,
    SquareParametrization,
    TanhParametrization,
    TanhSqParametrization,
)
from .result import Result

__version__ = '0.1.0'

__all__ = [
    'ControlFunction',
    'LinearParametrization',
    'Objective',
    'Parametrization',
    'Power',
    'PulseGradient',
    'QuadraticStateConstraint',
    'Result',
    'SquareParametrization',
    'StateDependentConstraint',
    'TanhParametrization',
    'TanhSqParametrization',
    'constraints',
    'convergence',
    'conversions',
    'ensemble_objectives',
    'functionals',
    'gate_objectives',
    'info_hooks',
    'mu',
    'nonlinear',
    'objectives',
    'optimize_pulses',
    'optimize_pulses_batch',
    'parallelization',
    'parametrization',
    'propagate_objectives',
    'propagators',
    'result',
    'second_order',
    'shapes',
]
