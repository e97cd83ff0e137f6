"""Cases, parameters and fp64 references of tests/test_trajhead_host.py and tests/test_gpu_trajhead.py: the classifier head of a
whole trajectory [T, N, C, H, W] in one call (odenet.py `FCClassifier.forward`, `head_on_trajectory`), the loss of the accuracy
sweep per slice (head.py `trajectory_loss`, csrc/kernels_loss.hip `k_head_loss_slices_fwd`), the sliced `norm='batch'` head
(head.py `bn_head_pool_slices`, csrc/kernels_bnhead.hip) and the trajectory distance of `attack diff` (head.py
`trajectory_distance`, csrc/kernels_head.hip `k_gn_relu_distance_*`).

The references are the reference's module sequences as `.double()` on the CPU, slice by slice (model.py:39-40 applies the head to
one slice at a time; adversarial/diff.py:111-123 forms the two distances from `relu(norm(slice))`).  Every tensor comes from a
generator seeded by the case, so the CPU and the GPU file see the same numbers."""
import functools

import torch
from torch import nn
from torch.nn import functional as F

# (T, N, C, H, W)
CPU_HEAD_CASES = [(3, 2, 64, 5, 5), (2, 3, 16, 7, 7)]
GN_HEAD_CASES = [(3, 2, 64, 8, 8), (4, 3, 64, 7, 7), (2, 5, 256, 8, 8)]      # 7 x 7: H W % 4 != 0, the one-thread-per-channel kernel
GN_HEAD_OUTS = [10, 200, None]                                                # Linear to 10 and to 200 classes, pool only
BN_HEAD_CASES = [(3, 2, 64, 8, 8), (2, 3, 64, 7, 7), (2, 84, 64, 7, 7), (3, 2, 192, 8, 8)]     # 84 samples: 21 chunks per slice
BN_OFFSET_CASE = (3, 4, 64, 8, 8)       # z = 50 + randn, slice s a further 10 s: statistics leaking between slices would show
# (T, N, C, classes): N % 4 != 0 (a workgroup holds four samples: slices must not share its partial), many classes, the sweep's 21 slices, one sample
LOSS_CASES = [(3, 5, 64, 10), (2, 4, 256, 200), (21, 7, 64, 10), (1, 1, 64, 10)]
DIST_CASES = [(3, 2, 64, 8, 8), (2, 3, 64, 7, 7), (5, 1, 256, 8, 8)]
# the fp32 chain of tensor operations' own error against fp64 at DIST_CASES on an MI355X, its worst case (tests/test_gpu_trajhead.py
# measures it in every run and prints it): relative in l2, absolute in cos
CHAIN_L2_REL, CHAIN_COS_ABS = 6.9e-8, 1.4e-7
POOLED_FLOOR = 1e-5                     # tests/bnhead_cases.py FLOORS['pooled']: the project's bound for this head


def seed_of(case):
    return 1000 + sum((k + 1) * int(v) for k, v in enumerate(case))


def trajectory(case, offset=0.0, slice_shift=0.0):
    """[T, N, C, H, W] fp32: randn (+ offset, + slice_shift * t for slice t)"""
    gen = torch.Generator().manual_seed(seed_of(case))
    x = torch.randn(*case, generator=gen) + offset
    if slice_shift:
        x = x + slice_shift * torch.arange(case[0], dtype=torch.float32).reshape(-1, 1, 1, 1, 1)
    return x


def perturb_(module, seed):
    """the norm's (and the Linear layer's) parameters moved off their initial values by 0.2 randn"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=gen))
    return module


def classifier(c, out, norm='group', features=False, seed=0):
    """an `FCClassifier` with perturbed parameters; features: the classification layer removed as `to_features_extractor` does"""
    import neural_ode_features_amd as nof
    torch.manual_seed(seed)
    head = perturb_(nof.FCClassifier(in_ch=c, out=out if out else 10, norm=norm), seed + 1)
    if features or out is None:
        head.module[-1] = nn.Sequential()
    return head.eval()


def group_norm(c, seed=0):
    torch.manual_seed(seed)
    return perturb_(nn.GroupNorm(min(32, c), c), seed + 1)


def pooled_fp64(head, x):
    """dropout-free `FCClassifier` body in front of the last layer, fp64 on the CPU, slice by slice: [T, N, C]"""
    norm = head.module[0]
    ref = type(norm)(norm.num_groups, norm.num_channels) if isinstance(norm, nn.GroupNorm) else nn.BatchNorm2d(norm.num_features, track_running_stats=False)
    ref = ref.double()
    ref.load_state_dict({k: v.double() for k, v in norm.state_dict().items()})
    with torch.no_grad():
        return torch.stack([F.adaptive_avg_pool2d(torch.relu(ref(xi.double())), (1, 1)).flatten(1) for xi in x.cpu()])


def loss_fp64(logits, target):
    """([T] summed cross-entropy, [T] arg-max hits) by an explicit loop over slices and samples, fp64"""
    lg, tg = logits.detach().cpu().double(), target.cpu()
    T, n, _ = lg.shape
    loss, hits = torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.float64)
    for t in range(T):
        for i in range(n):
            row = lg[t, i]
            loss[t] += torch.logsumexp(row, 0) - row[tg[i]]
            hits[t] += float(int(row.argmax()) == int(tg[i]))
    return loss, hits


def loss_inputs(case):
    """(pooled [T, N, C], weight [classes, C], bias [classes], target [N])"""
    T, n, c, o = case
    gen = torch.Generator().manual_seed(seed_of(case))
    pooled = torch.rand(T, n, c, generator=gen)
    weight = torch.randn(o, c, generator=gen) / c ** 0.5
    bias = 0.1 * torch.randn(o, generator=gen)
    target = torch.randint(0, o, (n,), generator=gen)
    return pooled, weight, bias, target


def distance_fp64(traj0, traj1, norm):
    """(l2, cos), each [T, N], of diff.py:111-123 in fp64 on the CPU: the head's norm + ReLU slice by slice, flattened per sample"""
    ref = nn.GroupNorm(norm.num_groups, norm.num_channels, eps=norm.eps).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in norm.state_dict().items()})
    T, n = traj0.shape[:2]
    with torch.no_grad():
        u0 = torch.stack([torch.relu(ref(v.double())) for v in traj0.cpu()]).reshape(T, n, -1)
        u1 = torch.stack([torch.relu(ref(v.double())) for v in traj1.cpu()]).reshape(T, n, -1)
        l2 = torch.zeros(T, n, dtype=torch.float64)
        cos = torch.zeros(T, n, dtype=torch.float64)
        for t in range(T):
            for i in range(n):
                a, b = u0[t, i], u1[t, i]
                l2[t, i] = ((b - a) ** 2).sum().sqrt()
                cos[t, i] = (a * b).sum() / (max(float(a.norm()), 1e-8) * max(float(b.norm()), 1e-8))
    return l2, cos


def aten_distance(traj0, traj1, norm):
    """what `attack diff` did before the kernel (attack.py, diff.py:111-123), on the tensors' own device in fp32"""
    T, n = traj0.shape[:2]
    with torch.no_grad():
        u0 = torch.stack([torch.relu(norm(v)) for v in traj0]).reshape(T, n, -1).transpose(0, 1)
        u1 = torch.stack([torch.relu(norm(v)) for v in traj1]).reshape(T, n, -1).transpose(0, 1)
        l2 = (u1 - u0).pow(2).sum(-1).sqrt()
        cos = F.cosine_similarity(u1, u0, dim=-1)
    return l2.t(), cos.t()


@functools.lru_cache(maxsize=None)
def distance_case(case):
    """(traj0, traj1 = traj0 + 0.05 randn, norm, fp64 l2, fp64 cos), computed once and shared"""
    traj0 = trajectory(case)
    gen = torch.Generator().manual_seed(seed_of(case) + 7)
    traj1 = traj0 + 0.05 * torch.randn(*case, generator=gen)
    norm = group_norm(case[2], seed_of(case))
    return (traj0, traj1, norm) + distance_fp64(traj0, traj1, norm)


class Trajectory(nn.Module):
    """stands in for the ODE block on the CPU: a trajectory of `t` fixed affine images of its input (no solve: the head is what is
    tested)"""
    nfe = 0

    def __init__(self, t=3):
        super().__init__()
        self.t = t
        self.return_last_only = True

    def forward(self, x):
        if self.return_last_only:
            return x * (1.0 + 0.5 * (self.t - 1)) + 0.1 * (self.t - 1)
        return torch.stack([x * (1.0 + 0.5 * k) + 0.1 * k for k in range(self.t)])
