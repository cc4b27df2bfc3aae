"""Result.dump(..., reference=True): a dump the REFERENCE can load (write direction).

Part 1 runs anywhere (no GPU, no reference): the file names only classes / functions that exist in an environment
with the reference and NumPy 1.x or 2.x installed, and this package's own Result.load reads it back.

Part 2 checks against what the REAL ``krotov`` package did with such a dump (QuTiP & friends stubbed;
``tests/golden/make_reference_goldens.py dump_continue`` ran it and stored the result in tests/golden/): it loaded the
file with its own ``krotov.result.Result.load`` and CONTINUED the optimisation with its own
``optimize_pulses(..., continue_from=...)``; the pulses it arrived at must be the ones this package arrives at when it
continues the same result itself."""
import os
import pickle
import pickletools
import sys
import time

import numpy as np
import pytest

import krotov_amd
from krotov_amd import configs

from helpers import DUMP_CONTINUE_CASES, numpy_plugins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

ALLOWED_GLOBALS = {
    'krotov.result Result', 'krotov.objectives _Objective_reduce_init', 'krotov.objectives _ControlPlaceholder',
    'numpy.core.multiarray _reconstruct', 'numpy ndarray', 'numpy dtype', 'time struct_time', '_codecs encode',
    '__builtin__ complex', 'builtins complex',
}


def _run_here(spec, iter_stop, continue_from=None):
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    prop, mu, overlap = numpy_plugins(spec.is_super)
    return objectives, krotov_amd.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=prop,
        chi_constructor=getattr(krotov_amd.functionals, 'chis_' + spec.chi), mu=mu, overlap=overlap,
        norm=np.linalg.norm, iter_stop=iter_stop, store_all_pulses=True, continue_from=continue_from)


@pytest.mark.parametrize('name', ['c1', 'c5_L3'])
def test_reference_format_dump_names_only_reference_classes(name, tmp_path):
    spec = configs.config_c1(nt=80) if name == 'c1' else configs.config_c5(K=3, N=6, nt=41, L=3, distinct=True)
    objectives, res = _run_here(spec, 2)
    path = str(tmp_path / 'result.dump')
    res.dump(path, reference=True)
    names = {arg for op, arg, _ in pickletools.genops(open(path, 'rb').read()) if op.name == 'GLOBAL'}
    assert names <= ALLOWED_GLOBALS, names - ALLOWED_GLOBALS
    assert {'krotov.result Result', 'krotov.objectives _Objective_reduce_init',
            'krotov.objectives _ControlPlaceholder'} <= names
    assert 'krotov' not in sys.modules  # (the stand-in modules of the dump are gone again)
    back = krotov_amd.result.Result.load(path, objectives=objectives)
    assert back.iters == res.iters and back.message == res.message
    assert np.array_equal(np.array(back.optimized_controls), np.array(res.optimized_controls))
    assert np.array_equal(np.array(back.all_pulses), np.array(res.all_pulses))
    assert np.allclose(np.array(back.tau_vals, dtype=complex), np.array(res.tau_vals, dtype=complex), atol=0, rtol=0)
    assert np.array_equal(back.tlist, spec.tlist)
    # without `objectives`: the stored ones come back with placeholders where the control functions were
    stored = krotov_amd.result.Result.load(path)
    assert len(stored.objectives) == spec.K
    assert isinstance(stored.objectives[0].H[1][1], krotov_amd.result.ControlPlaceholder)
    assert np.array_equal(np.asarray(stored.objectives[0].H[0]), np.asarray(objectives[0].H[0]))


def test_reference_format_dump_turns_numpy_scalars_into_python_scalars(tmp_path):
    """np.float64 / np.complex128 inherit from float / complex; left alone they are pickled under
    numpy._core.multiarray.scalar, which a NumPy-1.x (QuTiP 4) environment cannot resolve."""
    spec = configs.config_c1(nt=40)
    objectives, res = _run_here(spec, 1)
    res.info_vals = [np.float64(0.25), (np.float32(1.5), np.int64(3), [np.complex128(1 - 2j)])]
    res.tau_vals = [[np.complex128(0.5 + 0.25j)], np.array([np.complex128(1j)], dtype=object)]
    res.iter_seconds = [np.int32(0), np.float64(2.0)]
    path = str(tmp_path / 'scalars.dump')
    res.dump(path, reference=True)
    names = {arg for op, arg, _ in pickletools.genops(open(path, 'rb').read()) if op.name == 'GLOBAL'}
    assert names <= ALLOWED_GLOBALS, names - ALLOWED_GLOBALS
    back = krotov_amd.result.Result.load(path, objectives=objectives)
    assert type(back.info_vals[0]) is float and back.info_vals[0] == 0.25
    assert [type(v) for v in back.info_vals[1][:2]] == [float, int] and type(back.info_vals[1][2][0]) is complex
    assert type(back.tau_vals[0][0]) is complex and back.tau_vals[0][0] == 0.5 + 0.25j
    assert type(back.tau_vals[1][0]) is complex and back.tau_vals[1][0] == 1j
    assert [type(v) for v in back.iter_seconds] == [int, float]


def _globals(path):
    with open(path, 'rb') as fh:
        return {arg for op, arg, _ in pickletools.genops(fh.read()) if op.name == 'GLOBAL'}


class _Opaque:
    """Stand-in for every class or function a dump names, except NumPy's array pieces and the builtins: keeps what the
    unpickler hands it (constructor arguments, state), so that two dumps can be compared by structure."""

    def __init__(self, *args):
        self.args = args

    def __setstate__(self, state):
        self.state = state


class _StructureUnpickler(pickle.Unpickler):
    REAL = {('numpy.core.multiarray', '_reconstruct'), ('numpy._core.multiarray', '_reconstruct'), ('numpy', 'ndarray'),
            ('numpy', 'dtype'), ('time', 'struct_time'), ('_codecs', 'encode'), ('builtins', 'complex'),
            ('__builtin__', 'complex')}

    def find_class(self, module, name):
        if (module, name) in self.REAL:
            if module == '__builtin__':
                module = 'builtins'
            if module == 'numpy.core.multiarray' and hasattr(np, '_core'):
                module = 'numpy._core.multiarray'
            return super().find_class(module, name)
        return type('%s.%s' % (module, name), (_Opaque,), {})


def _structure(x):
    """What a loader meets in a dump, without the numbers: class names, attribute names, nesting, lengths, array dtypes
    and shapes, scalar types, strings (the local-time stamps only as such: they depend on when and where)."""
    if isinstance(x, _Opaque):
        return (type(x).__name__, _structure(getattr(x, 'args', None)), _structure(getattr(x, 'state', None)))
    if isinstance(x, dict):
        return ('dict', tuple((k, _structure(x[k])) for k in sorted(x, key=repr)))
    if isinstance(x, (list, tuple)) and not isinstance(x, time.struct_time):
        return (type(x).__name__, tuple(_structure(v) for v in x))
    if isinstance(x, np.ndarray):
        return ('ndarray', x.dtype.str, x.shape)
    if isinstance(x, str):
        return ('str', x)
    return (type(x).__name__,)


def _load_structure(path):
    with open(path, 'rb') as fh:
        return _structure(_StructureUnpickler(fh).load())


@pytest.mark.parametrize('name', sorted(DUMP_CONTINUE_CASES))
def test_the_reference_loads_the_dump_and_continues_it(name, tmp_path):
    """The reference's side is stored in tests/golden/ (``make_reference_goldens.py dump_continue``): the dump this package
    wrote after two iterations, which the reference's own ``Result.load`` read, and the controls the reference's
    ``optimize_pulses(..., continue_from=...)`` arrived at from it after four.  The dump written now must be that one
    (the same classes, functions, attributes, nesting, array shapes and types; the same numbers), and continuing it here
    must arrive at the reference's pulses."""
    spec = DUMP_CONTINUE_CASES[name](configs)
    objectives, res = _run_here(spec, 2)
    path = str(tmp_path / 'result.dump')
    res.dump(path, reference=True)
    shown = os.path.join(GOLDEN, 'reference_format_%s.dump' % name)
    assert _globals(path) == _globals(shown)
    assert _load_structure(path) == _load_structure(shown)
    now, then = (krotov_amd.result.Result.load(p, objectives=objectives) for p in (path, shown))
    assert now.iters == then.iters == [0, 1, 2] and now.message == then.message
    for field in ('optimized_controls', 'all_pulses'):
        a, b = np.array(getattr(now, field)), np.array(getattr(then, field))
        assert a.shape == b.shape and np.abs(a - b).max() < 1e-13 * max(1.0, np.abs(b).max()), field
    assert np.abs(np.array(now.tau_vals, dtype=complex) - np.array(then.tau_vals, dtype=complex)).max() < 1e-13
    assert np.array_equal(now.tlist, then.tlist)
    theirs = np.load(os.path.join(GOLDEN, 'ref_dump_continue.npz'))[name]
    _, mine = _run_here(spec, 4, continue_from=krotov_amd.result.Result.load(path, objectives=objectives))
    assert mine.iters == [0, 1, 2, 3, 4]
    assert np.abs(theirs - np.array(mine.optimized_controls)).max() < 1e-12 * max(1.0, np.abs(theirs).max())
