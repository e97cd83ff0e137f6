"""CPU: the basic-iterative attack's plain-torch loop (neural_ode_features_amd/attack.py: bim_reference -- what `bim` runs on CPU
tensors and what the GPU tests compare the kernels against) on a model whose attack can be followed by hand, plus the
command line's file handling.

The model: logits = W x.flatten() + b, W = [[1, -1, .5, 0], [-1, 1, 0, .5]], b = [.3, 0], fp64, no preprocessing, bounds
(0, 1); three 1 x 2 x 2 images, all labels 0, ten iterations.  The loss gradient of a two-class linear model with label 0 is
p1 (W1 - W0) = p1 [-2, 2, -.5, .5]: its sign pattern is (-, +, -, +) at every iterate, its direction is constant."""
import math
import os

import pytest
import torch

INF = float('inf')
W = torch.tensor([[1, -1, .5, 0], [-1, 1, 0, .5]], dtype=torch.float64)
B = torch.tensor([.3, 0], dtype=torch.float64)
X = torch.tensor([[.2, .5, .9, 0], [.9, .1, .5, .5], [.1, .9, .5, .5]], dtype=torch.float64).reshape(3, 1, 2, 2)
Y = torch.zeros(3, dtype=torch.int64)


def model(x):
    return x.flatten(1) @ W.t() + B


def _close(got, want):
    return float((got.flatten() - torch.tensor(want, dtype=torch.float64)).abs().max())


def test_linf_attack_matches_the_hand_computed_run():
    from neural_ode_features_amd.attack import bim
    r = bim(model, X, Y, norm=INF, epsilon=.25, stepsize=.1, iterations=10)
    # sample 0: one step of .1 against the gradient's sign flips the prediction
    assert _close(r.adversarial[0], [.1, .6, .8, .1]) <= 1e-12
    assert abs(float(r.distance[0]) - 0.1) <= 1e-12
    assert (int(r.original_class[0]), int(r.adversarial_class[0]), int(r.found_iteration[0])) == (0, 1, 1)
    # sample 1: saturates on the eps-ball without ever being misclassified
    assert _close(r.adversarial[1], [.65, .35, .25, .75]) <= 1e-12
    assert float(r.distance[1]) == INF and int(r.adversarial_class[1]) == -1 and int(r.found_iteration[1]) == -1
    assert int(r.original_class[1]) == 0
    # sample 2: a natural error -- never stepped
    assert torch.equal(r.adversarial[2], X[2])
    assert float(r.distance[2]) == 0.0
    assert (int(r.original_class[2]), int(r.adversarial_class[2]), int(r.found_iteration[2])) == (1, 1, 0)


def test_l2_attack_matches_the_hand_computed_run():
    from neural_ode_features_amd.attack import bim
    r = bim(model, X, Y, norm=2, epsilon=.2, stepsize=.1, iterations=10)
    assert _close(r.adversarial[0], [0.0628011319, 0.6371988681, 0.8657002830, 0.0342997170]) <= 1e-10
    # (the issue's digits are given to 1e-10; the closed form pins them to 1e-12: a step of rms .1 along [-2, 2, -.5, .5] / rms)
    d = torch.tensor([-2, 2, -.5, .5], dtype=torch.float64)
    d = d / d.pow(2).mean().sqrt()
    assert float((r.adversarial[0].flatten() - (X[0].flatten() + .1 * d)).abs().max()) <= 1e-12
    assert abs(float(r.distance[0]) - 0.01) <= 1e-12
    assert (int(r.adversarial_class[0]), int(r.found_iteration[0])) == (1, 1)
    assert _close(r.adversarial[1], [0.6256022638, 0.3743977362, 0.4314005659, 0.5685994341]) <= 1e-10
    assert float((r.adversarial[1].flatten() - (X[1].flatten() + .2 * d)).abs().max()) <= 1e-12
    p = r.adversarial[1] - X[1]
    assert abs(float(p.pow(2).mean().sqrt()) - 0.2) <= 1e-12          # the root-MEAN-square of the perturbation is epsilon
    assert float(r.distance[1]) == INF and int(r.adversarial_class[1]) == -1
    assert torch.equal(r.adversarial[2], X[2]) and float(r.distance[2]) == 0.0 and int(r.adversarial_class[2]) == 1


def test_return_early_off_keeps_the_smallest_distance():
    """Without return_early a found sample goes on stepping (its distance grows towards the eps-ball), and the record stays
    the first, smallest one; the natural error is still never stepped."""
    from neural_ode_features_amd.attack import bim, bim_reference
    for norm, eps, dist in ((INF, .25, 0.1), (2, .2, 0.01)):
        r = bim(model, X, Y, norm=norm, epsilon=eps, stepsize=.1, iterations=10, return_early=False)
        e = bim(model, X, Y, norm=norm, epsilon=eps, stepsize=.1, iterations=10, return_early=True)
        assert abs(float(r.distance[0]) - dist) <= 1e-12 and int(r.found_iteration[0]) == 1
        assert torch.equal(r.adversarial[0], e.adversarial[0])
        assert torch.equal(r.adversarial[2], X[2]) and int(r.found_iteration[2]) == 0
        assert torch.equal(r.adversarial[1], e.adversarial[1])
    # a model that is fooled only while the perturbation is SMALL in one pixel: later, larger iterates are misclassified too and
    # must not replace the record
    calls = []

    def spy(x):
        calls.append(x.detach().clone())
        return model(x)
    r = bim_reference(spy, X[:1], Y[:1], norm=INF, epsilon=.25, stepsize=.1, iterations=4, return_early=False)
    assert len(calls) == 5                                              # iterations + 1 forwards
    later = (calls[-1] - X[:1]).abs().max()
    assert float(later) > 0.1 + 1e-9 and abs(float(r.distance[0]) - 0.1) <= 1e-12


def test_preprocessing_goes_through_the_gradient():
    """(x - mean) / std in front of the model: the same attack as on a model that normalises inside."""
    from neural_ode_features_amd.attack import bim
    mean, std = (0.3,), (0.5,)
    inner = lambda z: model(z * 0.5 + 0.3)
    a = bim(inner, X, Y, norm=2, epsilon=.2, stepsize=.1, iterations=3, preprocessing=(mean, std))
    b = bim(model, X, Y, norm=2, epsilon=.2, stepsize=.1, iterations=3)
    assert float((a.adversarial - b.adversarial).abs().max()) <= 1e-12
    assert torch.equal(a.adversarial_class, b.adversarial_class)


def test_arguments_and_refusals():
    from neural_ode_features_amd import attack
    a = attack.build_parser().parse_args(['attack', 'some/run', '-t', '1e-3', '-e', '0.05', '-d', '2', '-s', '0.01', '--batch-size', '1',
                                          '--limit', '8'])
    assert (a.mode, a.run, a.tol, a.epsilon, a.distance, a.stepsize, a.batch_size, a.limit) == ('attack', 'some/run', 1e-3, .05, 2.0, .01, 1, 8)
    a = attack.build_parser().parse_args(['diff', 'r', '-d', 'inf'])
    assert a.distance == INF and a.tol is None and a.resolution == 50 and a.stepsize == 0.05
    with pytest.raises(SystemExit):
        attack.build_parser().parse_args(['attack', 'r', '-d', '1'])
    with pytest.raises(ValueError):
        attack.bim(model, X, Y, norm=1, epsilon=.1, stepsize=.1)
    with pytest.raises(ValueError):
        attack.bim(model, X, Y[:2], epsilon=.1, stepsize=.1)
    with pytest.raises(SystemExit, match=r'\[0, 1\]'):
        attack.unit_images(torch.tensor([[-0.5, 2.0]]))
    assert torch.equal(attack.unit_images(torch.tensor([0, 255], dtype=torch.uint8)), torch.tensor([0.0, 1.0]))
    d = attack.sub_dir('run', 1e-3, .05, 2.0, .01)
    assert d.startswith(os.path.join('run', 'adv-attack')) and d != attack.sub_dir('run', 1e-3, .05, INF, .01)


def test_results_csv_and_skip_if_present(tmp_path):
    from neural_ode_features_amd import attack
    path = str(tmp_path / 'results.csv')
    assert attack.read_results(path) == {} and attack.pending(4, {}) == [0, 1, 2, 3]
    rows = [dict(sample_id=0, label=3, elapsed_time=.5, distance=0.01, adversarial_class=4, original_class=3),
            dict(sample_id=2, label=1, elapsed_time=.5, distance=INF, adversarial_class=float('nan'), original_class=1)]
    attack.append_rows(path, rows)
    with open(path) as fh:
        assert fh.readline().strip().split(',') == list(attack.COLUMNS)
    done = attack.read_results(path)
    assert sorted(done) == [0, 2] and attack.pending(4, done) == [1, 3]
    assert done[0]['distance'] == 0.01 and math.isinf(done[2]['distance']) and math.isnan(done[2]['adversarial_class'])
    attack.append_rows(path, [dict(sample_id=1, label=0, elapsed_time=.1, distance=0.0, adversarial_class=5, original_class=5)])
    with open(path) as fh:
        lines = fh.read().strip().splitlines()
    assert len(lines) == 4 and lines[0].split(',') == list(attack.COLUMNS)          # one header, three rows
    assert attack.pending(4, attack.read_results(path)) == [3]
