"""The guarded allocator of tests/guarded.py catches what it is for (CPU only: the device filter opened to CPU tensors).

Four fake "nodes", plain Python functions on `torch.empty` outputs and a `workspace.alloc`'d workspace, each with one of
the faults the guard-band tests of test_gpu_guard_bands.py look for; the checks of that file (guarded.guarded_run) must
fail for each with a message that names the cause, and pass for the correct fake.
"""
import pytest
import torch

from neural_ode_features_amd import workspace
from tests import guarded as G

N = 37          # ragged on purpose: no multiple of anything
PAST = float(torch.tensor(0x11223344, dtype=torch.int32).view(torch.float32))


def _build():
    gen = torch.Generator().manual_seed(5)
    return [torch.rand(N, generator=gen) + 0.5]          # positive: fmax(x, 0) == x, so the zero fill hides fault (c) as a zeroed workspace would


def _scratch(ws):
    return ws[:N * 4].view(torch.float32)


def node_correct(ts):
    x, = ts
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace.alloc(N * 4, x.device)
    s = _scratch(ws)
    s.copy_(x * 2)
    out.copy_(torch.fmax(x, s))
    return [out]


def node_writes_past_output(ts):          # (a)
    out, = node_correct(ts)
    torch.as_strided(out, (N + 1,), (1,))[N] = PAST          # every byte of it differs from every fill
    return [out]


def node_leaves_last_unwritten(ts):       # (b)
    x, = ts
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace.alloc(N * 4, x.device)
    s = _scratch(ws)
    s.copy_(x * 2)
    out[:N - 1].copy_(torch.fmax(x, s)[:N - 1])
    return [out]


def node_reads_unwritten_workspace(ts):   # (c)
    x, = ts
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace.alloc(N * 4, x.device)
    s = _scratch(ws)
    s[:N - 1].copy_(x[:N - 1] * 2)                      # s[N-1] is read below and was never written
    # the maximum as kernels compute it (fmaxf: a NaN operand is dropped).  torch.maximum would propagate the NaN and so
    # show the fault under the NaN fill too; the point here is the fault that only the finite fill shows
    out.copy_(torch.fmax(x * 2, s))
    return [out]


def node_writes_slack(ts):                # (d)
    x, = ts
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = workspace.alloc(N * 4, x.device)
    s = _scratch(ws)
    s.copy_(x * 2)
    ws[N * 4 + 3] = 0x11                                 # inside the 256 bytes workspace.alloc adds: not the library's
    out.copy_(torch.fmax(x, s))
    return [out]


def _case(run):
    return G.Case(run.__name__, _build, run, workspaces=lambda ts: [N * 4], outputs=[((N,), torch.float32)])


@pytest.fixture(scope='module')
def plain():
    return G.plain_run(_case(node_correct), 'cpu')


def test_correct_fake_passes(plain):
    for fill in G.FILLS:
        g = G.guarded_run(_case(node_correct), fill, plain, 'cpu')
        assert g.workspaces == [N * 4] and g.outputs == [((N,), torch.float32)]
    G.verify(_case(node_correct), 'cpu')


@pytest.mark.parametrize('fill', G.FILLS)
def test_write_past_output_is_a_band_hit(plain, fill):
    with pytest.raises(AssertionError) as e:
        G.guarded_run(_case(node_writes_past_output), fill, plain, 'cpu')
    msg = str(e.value)
    assert 'float32 tensor of shape (37,)' in msg and 'right band written' in msg and 'at byte offset %d (0 past its %d bytes)' % (N * 4, N * 4) in msg


@pytest.mark.parametrize('fill', G.FILLS)
def test_unwritten_element_changes_a_result(plain, fill):
    with pytest.raises(AssertionError) as e:
        G.guarded_run(_case(node_leaves_last_unwritten), fill, plain, 'cpu')
    msg = str(e.value)
    assert 'result 0 depends on bytes the node does not own' in msg and 'fill 0x%02X' % fill in msg
    assert '1 of 37 elements differ, first at flat index 36' in msg


def test_uninitialised_workspace_read_shows_under_the_finite_fill_only(plain):
    case = _case(node_reads_unwritten_workspace)
    G.guarded_run(case, 0xFF, plain, 'cpu')          # fmax drops the NaN
    G.guarded_run(case, 0x00, plain, 'cpu')          # inputs are positive
    with pytest.raises(AssertionError) as e:
        G.guarded_run(case, 0x7F, plain, 'cpu')
    msg = str(e.value)
    assert 'result 0 depends on bytes the node does not own' in msg and 'fill 0x7F' in msg and 'first at flat index 36' in msg
    with pytest.raises(AssertionError):
        for fill in G.FILLS:
            G.guarded_run(case, fill, plain, 'cpu')


@pytest.mark.parametrize('fill', G.FILLS)
def test_write_into_the_slack_is_a_band_hit(plain, fill):
    with pytest.raises(AssertionError) as e:
        G.guarded_run(_case(node_writes_slack), fill, plain, 'cpu')
    msg = str(e.value)
    assert 'workspace of %d bytes' % (N * 4) in msg and 'slack behind nbytes written' in msg and '(3 past its %d bytes)' % (N * 4) in msg


def test_a_node_that_did_not_run_fails():
    """A wrapper that fell back to another path allocates no workspace of the planned size."""
    def fallback(ts):
        return [torch.fmax(ts[0], ts[0] * 2)]
    plain = G.plain_run(_case(fallback), 'cpu')
    with pytest.raises(AssertionError, match='did not run its HIP node'):
        G.guarded_run(_case(fallback), 0xFF, plain, 'cpu')
    with pytest.raises(AssertionError, match='no torch.float32 output of shape'):
        G.guarded_run(G.Case('fallback', _build, fallback, outputs=[((N,), torch.float32)]), 0xFF, plain, 'cpu')


def test_library_calls_and_planned_bytes_are_demanded(plain):
    from neural_ode_features_amd import _lib
    lib = _lib.load()
    real = lib.node_retrieval_workspace_bytes
    planned = real(5, 7, 20)
    assert planned > 0

    def node(ts):
        out, = node_correct(ts)
        workspace.alloc(lib.node_retrieval_workspace_bytes(5, 7, 20), ts[0].device)
        return [out]

    def node_other_size(ts):
        out, = node_correct(ts)
        workspace.alloc(lib.node_retrieval_workspace_bytes(5, 7, 20) + 4, ts[0].device)
        return [out]
    G.guarded_run(G.Case('planned', _build, node, bytes_fn='node_retrieval_workspace_bytes', calls=['node_retrieval_workspace_bytes']), 0xFF, plain, 'cpu')
    assert lib.node_retrieval_workspace_bytes is real
    with pytest.raises(AssertionError, match='no workspace of exactly that size was allocated'):
        G.guarded_run(G.Case('other', _build, node_other_size, bytes_fn='node_retrieval_workspace_bytes'), 0xFF, plain, 'cpu')
    with pytest.raises(AssertionError, match='node_rank_ap was never called'):
        G.guarded_run(G.Case('uncalled', _build, node, calls=['node_rank_ap']), 0xFF, plain, 'cpu')
    assert lib.node_rank_ap is not None and lib.node_retrieval_workspace_bytes is real


def test_changed_input_and_its_bands_are_reported(plain):
    def scribbles(ts):
        ts[0][0] = 3.0
        return node_correct(ts)
    with pytest.raises(AssertionError, match='an input was changed by the call'):
        G.guarded_run(_case(scribbles), 0x7F, plain, 'cpu', compare=False)

    def underruns(ts):
        torch.as_strided(ts[0], (1,), (1,), ts[0].storage_offset() - 1)[0] = 3.0
        return node_correct(ts)
    with pytest.raises(AssertionError, match='bands around an input were written: input float32 of shape .37,.: left band written'):
        G.guarded_run(_case(underruns), 0x7F, plain, 'cpu')


def test_patch_and_restore_leave_the_original_objects():
    empty, empty_like, zeros, alloc = torch.empty, torch.empty_like, torch.zeros, workspace.alloc
    with G.guarded(0xFF, device_type='cpu'):
        assert torch.empty is not empty and workspace.alloc is not alloc
    assert torch.empty is empty and torch.empty_like is empty_like and torch.zeros is zeros and workspace.alloc is alloc
    with pytest.raises(RuntimeError):
        with G.guarded(0xFF, device_type='cpu'):
            raise RuntimeError('inside')
    assert torch.empty is empty and torch.empty_like is empty_like and torch.zeros is zeros and workspace.alloc is alloc


def test_cpu_and_non_contiguous_requests_fall_through_under_the_cuda_filter():
    with G.guarded(0x7F) as g:                      # the filter the GPU tests use
        a = torch.empty(3, 4)
        b = torch.empty((3, 4), dtype=torch.float64, device='cpu')
        c = torch.empty_like(b)
        d = torch.zeros(5, device='cpu')
        e = torch.empty(2, 3, 4, 5, device='cpu', memory_format=torch.channels_last)
        assert not g.regions and not g.outputs
        assert a.shape == (3, 4) and c.dtype == torch.float64 and not d.any() and e.is_contiguous(memory_format=torch.channels_last)
    strided = torch.empty(4, 6).t()
    with G.guarded(0x7F, device_type='cpu') as g:   # opened to the CPU: channels_last and strided sources still fall through
        e = torch.empty(2, 3, 4, 5, device='cpu', memory_format=torch.channels_last)
        f = torch.empty_like(strided)
        assert not g.regions and f.stride() == (1, 6)
        h = torch.empty_like(b)
        assert len(g.regions) == 1 and h.data_ptr() % 256 == 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64])
def test_every_dtype_gets_an_aligned_body_of_fill_between_bands(dtype):
    with G.guarded(0x7F, device_type='cpu') as g:
        t = torch.empty(3, 5, dtype=dtype, device='cpu')
        s = torch.empty((), dtype=dtype, device='cpu')
        z = torch.zeros(7, dtype=dtype, device='cpu')
        like = torch.empty_like(t)
    for x in (t, s, z, like):
        assert x.dtype == dtype and x.data_ptr() % 256 == 0 and x.is_contiguous() and x._base is None
    assert bool((t.reshape(-1).view(torch.uint8) == 0x7F).all()) and not z.any()
    assert all(r.band >= G.MIN_BAND and r.band >= r.body_bytes for r in g.regions)
    g.check()
    z[6] = 1                                        # the body is the tensor's own
    g.check()


def test_workspace_is_aligned_and_exactly_bounded():
    with G.guarded(0xFF, device_type='cpu') as g:
        buf = workspace.alloc(1000, torch.device('cpu'))
        assert workspace.aligned_ptr(buf) == buf.data_ptr() and workspace.holds(buf, 1000) and buf.numel() == 1256
        buf[:1000] = 1
        g.check()
        buf[1000] = 1
        with pytest.raises(AssertionError, match=r'workspace of 1000 bytes: slack behind nbytes written.*\(0 past its 1000 bytes\)'):
            g.check()


def test_band_grows_with_the_body():
    with G.guarded(0x00, device_type='cpu') as g:
        torch.empty(3 << 19, dtype=torch.float32, device='cpu')       # 6 MiB
    assert g.regions[0].band >= 6 << 20


def test_guarded_tensor_may_leave_an_autograd_function():
    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = torch.empty_like(x)
            out.copy_(x * 2)
            return out

        @staticmethod
        def backward(ctx, g):
            d = torch.empty_like(g)
            d.copy_(g * 2)
            return d

    x = G.embed(torch.arange(6.0), 0xFF).requires_grad_(True)
    with G.guarded(0xFF, device_type='cpu') as g:
        (F.apply(x) * torch.arange(1.0, 7.0)).sum().backward()        # (a dense cotangent: sum() alone hands backward an expanded one)
    g.check()
    assert torch.equal(x.grad, 2 * torch.arange(1.0, 7.0)) and len(g.regions) == 2
