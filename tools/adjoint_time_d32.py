#!/usr/bin/env python
"""d32 of every case of tests/test_gpu_adjoint_time.py: how far the fp32 CPU oracle's time gradient lies from the fp64 arbiter's,
max_i |gt32_i - gt64_i| / max_i |gt64_i| (tests.helpers.adjoint_time_case).  The GPU test's bound on grad_t is 8 x the largest d32
of a kernel family, rounded up to one significant digit; nothing here runs a kernel of the package.  Also prints how well
conditioned each grad_t is: min_i |grad_t_i| / sum_j ||f_j|| ||g_j||.

    NODE_TEST_ARBITER=cpu python3 tools/adjoint_time_d32.py       # the table at the head of profiles/adjoint_time_grads.txt
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def round_up_1(x):
    """x rounded up to one significant digit."""
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def main():
    from tests.helpers import AT_DOPRI5, AT_FAMILIES, AT_RK4, adjoint_time_case, at_id
    worst = {}
    print('%-44s %10s %10s' % ('case', 'd32', 'cond'))
    for fam, grid, method, mode in AT_DOPRI5 + AT_RK4:
        c = adjoint_time_case(AT_FAMILIES[fam][0], grid, method, mode)
        print('%-44s %10.2e %10.2e' % (at_id(fam, grid, method, mode), c['d32'], c['cond']), flush=True)
        worst[(method, fam)] = max(worst.get((method, fam), 0.0), c['d32'])
    print('%-20s %10s %10s' % ('method, family', 'max d32', 'bound'))
    for (method, fam), d in worst.items():
        print('%-20s %10.2e %10.0e' % (method + ', ' + fam, d, round_up_1(8 * d)))


if __name__ == '__main__':
    main()
