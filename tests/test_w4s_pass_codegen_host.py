"""Host: the multiply-add contraction of the twelve k_w4s_pass instantiations is pinned.

The library is built with -ffp-contract=fast, and which multiplies and adds of the Winograd transforms become one fused instruction
depends on how the compiler pairs them into packed instructions -- which moved when the pass body was put behind a function boundary
(four v_pk_fma_f32 fewer per kernel, the last bit of every solve different; profiles/launch_diet_ab.txt, section 3).  The results of a
solve are compared bit for bit from commit to commit (bench.py --dump-outputs), so a change of these counts -- an edit of
kernels_w4s.hip / w4s_pass_body.inc, or a new compiler -- is a change of results and has to be a decision, not an accident: this
test compiles the file for gfx950 (no GPU needed) and counts.  Packed / scalar ADDS are not pinned: they round the same either way."""
import collections
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (HEAD, TAIL, Q) -> (v_pk_fma_f32, v_fma_f32 + v_fmac_f32, v_pk_mul_f32, v_mul_f32)
PINNED = {(0, 1, 1): (223, 74, 84, 39), (0, 1, 4): (223, 74, 84, 40), (1, 0, 1): (80, 54, 54, 46), (1, 0, 4): (80, 54, 54, 47),
          (1, 1, 1): (434, 82, 166, 50), (1, 1, 4): (434, 82, 166, 51), (1, 2, 1): (302, 79, 170, 89), (1, 2, 4): (252, 79, 190, 154),
          (2, 0, 1): (117, 99, 88, 65), (2, 0, 4): (116, 95, 88, 69), (2, 1, 1): (292, 121, 149, 81), (2, 1, 4): (292, 121, 149, 82)}


def test_pass_kernels_keep_their_contractions(tmp_path):
    spec = importlib.util.spec_from_file_location('node_amd_build', os.path.join(ROOT, 'neural-ode-features_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    asm = str(tmp_path / 'kernels_w4s.s')
    subprocess.check_call([b.HIPCC] + b.FLAGS + ['--cuda-device-only', '-S', os.path.join(b.CSRC, 'kernels_w4s.hip'), '-o', asm])
    got, cur = {}, None
    for line in open(asm):
        m = re.match(r'^_ZN4node10k_w4s_passILi(\d)ELi(\d)ELi(\d)EEEvNS_7W4sArgsE:', line)
        if m:
            cur = tuple(int(v) for v in m.groups())
            got[cur] = collections.Counter()
        elif line.startswith('.Lfunc_end'):
            cur = None
        elif cur is not None:
            t = line.split()
            if t:
                got[cur][t[0]] += 1
    counts = {k: (c['v_pk_fma_f32'], c['v_fma_f32'] + c['v_fmac_f32_e32'], c['v_pk_mul_f32'], c['v_mul_f32_e32']) for k, c in got.items()}
    assert counts == PINNED, {k: (counts.get(k), PINNED[k]) for k in PINNED if counts.get(k) != PINNED[k]}
