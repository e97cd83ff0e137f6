"""Caller-owned workspaces (workspace.py): every buffer handed out holds its bytes behind the aligned pointer, per-stream
scratch is per stream, and a carried workspace comes back from the pool instead of being allocated again."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _holds(buf, nbytes):
    from neural_ode_features_amd import workspace
    ptr = workspace.aligned_ptr(buf)
    return buf.numel() >= nbytes + 256 and ptr % 256 == 0 and ptr >= buf.data_ptr() \
        and ptr + nbytes <= buf.data_ptr() + buf.numel()


def test_scratch_grows_with_the_request_and_is_per_stream():
    from neural_ode_features_amd import workspace
    dev = torch.device('cuda', torch.cuda.current_device())
    ws = workspace.Scratch()
    small = ws.take(dev, 1000)
    assert _holds(small, 1000)
    large = ws.take(dev, 1200)          # 1256 bytes do not hold 1200 behind a pointer rounded up by up to 255
    assert _holds(large, 1200)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ws.take(dev, 1200)
    assert _holds(other, 1200) and other.data_ptr() != large.data_ptr()
    assert ws.take(dev, 500) is large and len(list(ws.values())) == 2
    assert ws.take(torch.device('cuda'), 500) is large          # no index: the current device
    assert ws.take(dev, 500, 7, 3) is not large                 # extra key parts (a shape) get a buffer of their own


def test_carried_pool_hands_out_one_buffer_per_forward_in_flight():
    from neural_ode_features_amd import workspace
    dev = torch.device('cuda', torch.cuda.current_device())
    pool = workspace.Carried()
    a = pool.take('k', dev, 1000)
    b = pool.take('k', dev, 1000)
    assert _holds(a, 1000) and _holds(b, 1000) and a.data_ptr() != b.data_ptr()
    ptrs = {a.data_ptr(), b.data_ptr()}
    pool.give('k', a)
    pool.give('k', b)
    c = pool.take('k', dev, 1000)
    assert c.data_ptr() in ptrs and (c is a or c is b)
    assert _holds(pool.take('k', dev, 4000), 4000)               # the free one is too small: a fresh buffer
    single = workspace.Carried(keep=1)
    single.give('k', a)
    single.give('k', b)
    assert len(single['k']) == 1 and single['k'][0] is b        # keep=1: the buffer given back last is the one kept
