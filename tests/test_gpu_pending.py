"""While a run is pending on a context (simplyp_run_async without its simplyp_sync), every analysis entry refuses: the entry
frame's timed bracket records the context's ev_start / ev_stop, and simplyp_sync reads exactly those events for the run's
kernel_ms and pilot_ms."""

import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import helpers
from simplyp_amd import engine

pytestmark = pytest.mark.gpu
PENDING = 'a run is pending on this context'


def _census():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'make_refusals.py')
    spec = importlib.util.spec_from_file_location('make_refusals', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_analysis_entry_refuses_while_a_run_is_pending(engine0):
    """Tarland 2004, one reach, 64 members, Engine.run(defer_sync=True) on a non-default torch stream.  Before finish() every
    analysis entry of the library, called through engine.lib() with this engine's handle, returns SIMPLYP_ERR_ARG with
    "<entry>: a run is pending on this context; call simplyp_sync first", which Engine._check raises as EngineError; nothing is
    launched.  The Engine methods themselves raise EngineError too, one call earlier: their first step, binding torch's
    stream (simplyp_ctx_set_stream), has always refused a pending context, with its own text "a run is pending; call simplyp_sync
    first".  Then finish(): the table equals, bit for bit, the table of the same run made without defer_sync, the work counters
    are equal, and kernel_ms is the run's.

    Before the entries shared one frame, simplyp_quantiles, simplyp_weighted_quantiles, simplyp_scores and simplyp_pareto did not
    look at the pending flag -- and simplyp_eval_units neither: for these five this test fails at the commit before."""
    import torch
    m = helpers.marshal_scenario('tarland_2004_static', E=64)
    rng = np.random.default_rng(11)
    m['member_params'][2] *= rng.uniform(0.9, 1.1, 64)
    args = (m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    ref, ref_status, ref_stats = engine0.run(*args)
    L = engine.lib()
    scratch = torch.zeros(4096, dtype=torch.float64, device=engine0.tdev)
    torch.cuda.synchronize()
    todo = _census().cases(engine0._h, scratch.data_ptr())
    todo.pop()
    first = {}
    for entry, label, a, info_class in todo:
        first.setdefault(entry, (a, info_class))
    assert len(first) == 27
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out, status, st = engine0.run(*args, defer_sync=True)
        for entry, (a, info_class) in first.items():
            info = None if info_class is None else info_class()
            rc = getattr(L, entry)(*(a if info is None else a + (C.byref(info),)))
            assert rc == -1, entry                                                     # SIMPLYP_ERR_ARG
            assert L.simplyp_last_error(engine0._h).decode() == '%s: %s; call simplyp_sync first' % (entry, PENDING)
            with pytest.raises(engine.EngineError, match=PENDING):
                engine0._check(rc, entry)
        row = out[0, 0]                                                                # [n_reaches, E]: never read
        for call in (lambda: engine0.quantiles(out, [0.5]),
                     lambda: engine0.weighted_quantiles(out, [0.5], np.ones(64, dtype=np.int64)),
                     lambda: engine0.scores(row, np.zeros(row.shape[0])),
                     lambda: engine0.pareto(row[:1].contiguous(), [1]),
                     lambda: engine0.eval_units('log', [[1.0]])):
            with pytest.raises(engine.EngineError, match='a run is pending'):
                call()
        st.update(st.pop('finish')())
    s.synchronize()
    assert not bool(scratch.any())
    assert bool(torch.equal(out, ref)) and bool(torch.equal(status, ref_status))
    for k in ('rhs_evals', 'steps', 'rejected'):
        assert st[k] == ref_stats[k], k
    assert st['kernel_ms'] > 0
