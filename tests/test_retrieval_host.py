"""CPU-side checks of the retrieval evaluation's boundary (csrc/retrieval_api.hip, retrieval.py): workspace sizes and
refusals of the C ABI, and the argument checks of the Python wrappers.  No compute: there is no GPU here."""
import pytest
import torch


def test_workspace_bytes_and_refusals():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    full = lib.node_retrieval_workspace_bytes(10000, 10000, 256)
    assert full > 0 and full % 256 == 0
    assert lib.node_retrieval_workspace_bytes(1, 1, 1) > 0
    assert lib.node_retrieval_workspace_bytes(10000, 16384, 256) > 0
    # the workspace holds one chunk of query rows: it stops growing with the number of queries
    assert lib.node_retrieval_workspace_bytes(100000, 10000, 256) == full
    for args, word in (((10000, 16385, 256), '16384'), ((10000, 10000, 0), 'd=0'), ((0, 10000, 256), 'nq=0')):
        assert lib.node_retrieval_workspace_bytes(*args) == 0, args
        assert word in lib.node_last_error().decode(), (args, lib.node_last_error())


def test_entry_points_refuse_before_touching_the_device():
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    dummy = 256      # never dereferenced: every refusal below happens on the host
    rc = lib.node_retrieval_ap(4, 16385, 8, dummy, dummy, dummy, dummy, 10, dummy, dummy, dummy, 1 << 20, None)
    assert rc == -3 and 'at most 16384' in lib.node_last_error().decode()                       # NODE_ERR_UNSUPPORTED
    rc = lib.node_rank_ap(4, 16385, dummy, dummy, dummy, 10, dummy, dummy, None, 0, None)
    assert rc == -3 and 'at most 16384' in lib.node_last_error().decode()
    rc = lib.node_rank_ap(4, 100, dummy, dummy, dummy, 0, dummy, dummy, None, 0, None)
    assert rc == -9 and 'k=0' in lib.node_last_error().decode()                                # NODE_ERR_ARG
    rc = lib.node_rank_ap(4, 100, None, dummy, dummy, 10, dummy, dummy, None, 0, None)
    assert rc == -1 and 'NULL' in lib.node_last_error().decode()                               # NODE_ERR_NULL
    rc = lib.node_retrieval_ap(4, 100, 8, dummy, dummy, dummy, dummy, 10, dummy, dummy, dummy, 16, None)
    assert rc == -4 and 'workspace too small' in lib.node_last_error().decode()                # NODE_ERR_WORKSPACE
    rc = lib.node_retrieval_ap(0, 100, 8, dummy, dummy, dummy, dummy, 10, dummy, dummy, dummy, 1 << 20, None)
    assert rc == -2 and 'nq=0' in lib.node_last_error().decode()                               # NODE_ERR_SHAPE


def test_python_wrappers_refuse_bad_arguments():
    from neural_ode_features_amd import retrieval as R
    q, x = torch.randn(5, 8), torch.randn(7, 8)
    lq, lx = torch.zeros(5, dtype=torch.int64), torch.zeros(7, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        R.average_precision(q, x, lq, lx)
    with pytest.raises(RuntimeError, match='no CPU path'):
        R.average_precision_from_scores(q @ x.T, lq, lx)
    for k in (0, -3, 2.5):
        with pytest.raises(ValueError, match='k must be an integer >= 1'):
            R.average_precision(q, x, lq, lx, k=k)
        with pytest.raises(ValueError, match='k must be an integer >= 1'):
            R.average_precision_from_scores(q @ x.T, lq, lx, k=k)
    with pytest.raises(TypeError, match='float32'):
        R.average_precision(q.double(), x.double(), lq, lx)
    with pytest.raises(TypeError, match='float32'):
        R.average_precision_from_scores((q @ x.T).half(), lq, lx)
    with pytest.raises(ValueError, match='contiguous'):
        R.average_precision(q, x.T.contiguous().T, lq, lx)
    with pytest.raises(ValueError, match='at most 16384'):
        R.average_precision_from_scores(torch.zeros(1, 16385), lq[:1], torch.zeros(16385, dtype=torch.int64))
