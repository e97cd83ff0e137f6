"""The step-count policy of deferred completion (`deferred.Deferred`), pinned on the host: how many steps a blind solve
enqueues after a given history of true counts, and when a key counts as settled.  No GPU: `Deferred` constructs on 'cpu'
and the policy is pure Python.  Also: the names `integrate` re-exports are the objects of their new homes."""
import copy

import pytest
import torch


KEY = ('fwd', 1, (2, 64, 8, 8), 1e-3, 1e-3, (0.0, 1.0))
COUNTS = [5, 5, 5, 6, 6, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5]
ENQUEUED = [6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 6, 5, 5, 5, 5]


def test_enqueue_counts_and_settling_follow_the_history():
    from neural_ode_features_amd.deferred import Deferred
    if (Deferred.HIST, Deferred.CALM, Deferred.FRAGILE, Deferred.QUIET) != (8, 4, 0.05, 8):
        pytest.skip('the policy constants are overridden in the environment')
    d = Deferred('cpu')
    d.armed = True
    d.learned(KEY, 5)
    seen = []
    for count in COUNTS:
        seen.append((d._enqueue(KEY), d.settled()))
        d._observe(KEY, count)
    assert [e for e, _ in seen] == ENQUEUED
    assert [s for _, s in seen] == [False] * 13 + [True] * 4

    d.forget()
    assert d.guess[KEY] is None and d.plan(KEY) is None
    d.learned(KEY, 4)
    d.force_counts(7)
    assert d._enqueue(KEY) == 7 and d.settled() is True and d.plan(KEY) == (7, 7)
    d.armed = False
    assert d.plan(KEY) is None


def test_integrate_reexports_the_moved_objects():
    from neural_ode_features_amd import deferred, integrate, recognise
    assert integrate.Deferred is deferred.Deferred and integrate.DeferredLoop is deferred.DeferredLoop
    assert integrate._func_token is deferred._func_token
    assert integrate.Recognised is recognise.Recognised and integrate.recognised is recognise.recognised


def test_a_deep_copy_gets_a_token_of_its_own():
    from neural_ode_features_amd.deferred import _func_token
    m = torch.nn.Linear(2, 2)
    twin = copy.deepcopy(m)
    assert _func_token(m) == _func_token(m) and _func_token(twin) != _func_token(m)
