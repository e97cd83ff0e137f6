"""Build recipe for libnode_hip.so (gfx950 only, in-tree).

    python neural-ode-features_amd/build.py [--force] [--diag]

`--diag` also links libnode_hip_diag.so: the same objects with DIAG_SOURCES compiled -DNODE_DIAG, i.e. WITH the in-kernel
stamps and the measured-and-rejected kernel variants (kernels_w4_diag.hip, which no other build compiles) that tools/ and the
`-m diag` tests use (NODE_HIP_DIAG=1 makes _lib.load() take it).  The product library contains none of them.

hipcc cross-compiles for gfx950 without a GPU; the built .so stays next to the
sources (git-ignored, but it travels to the GPU box with the gpurun snapshot).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
ROOT = os.path.dirname(HERE)
LIB = os.path.join(CSRC, 'libnode_hip.so')
LIB_DIAG = os.path.join(CSRC, 'libnode_hip_diag.so')
# translation units that hold `#ifdef NODE_DIAG` code (w4_gemm.h's stamps among it), and one that is not in SOURCES: diagnostics library only
DIAG_SOURCES = ['kernels_w4_bf16.hip', 'kernels_w4_f16.hip', 'w4_select.hip', 'kernels_w4_diag.hip', 'kernels_tiny_solve.hip']
SOURCES = ['kernels_layout.hip', 'kernels_groupnorm.hip', 'kernels_step_control.hip', 'kernels_generic.hip', 'kernels_theta_finalize.hip',
           'kernels_conv_direct.hip', 'kernels_conv_wino1d.hip', 'kernels_conv_wino2d.hip', 'kernels_conv_small.hip', 'conv_select.hip', 'kernels_wgrad.hip', 'kernels_head.hip', 'kernels_loss.hip', 'kernels_optim.hip', 'kernels_w4_pack.hip', 'kernels_w4_f32.hip', 'kernels_w4_bf16.hip', 'kernels_w4_f16.hip', 'kernels_w4_wgrad.hip', 'w4_select.hip', 'kernels_w4s.hip', 'kernels_stem.hip', 'kernels_stem_banded.hip', 'kernels_tiny.hip', 'kernels_tiny_solve.hip', 'kernels_retrieval.hip', 'kernels_svm.hip', 'kernels_augment.hip', 'kernels_resize.hip', 'kernels_imgconv.hip', 'kernels_pool.hip', 'kernels_ministem.hip', 'kernels_bnministem.hip', 'kernels_attack.hip', 'kernels_batchnorm.hip', 'kernels_bnhead.hip', 'bnfunc_api.hip', 'bnsolve_api.hip', 'bntrunk_api.hip', 'bnstem_api.hip', 'bnhead_api.hip', 'attack_api.hip', 'stem_api.hip', 'trunk_api.hip', 'downconv_api.hip', 'convstem_api.hip', 'bndownconv_api.hip', 'bnconvstem_api.hip','ministem_api.hip', 'bnministem_api.hip', 'retrieval_api.hip', 'svm_api.hip', 'augment_api.hip', 'resize_api.hip', 'imgconv_api.hip', 'pool_api.hip', 'host_common.hip', 'dims.hip', 'plan.hip', 'solver.hip', 'api_solve.hip',
           'api_backprop.hip', 'api_flat.hip', 'api_misc.hip']
HEADERS = [os.path.join(CSRC, 'node_internal.h'), os.path.join(CSRC, 'wino4.h'), os.path.join(CSRC, 'w4_gemm.h'), os.path.join(CSRC, 'theta_finalize.h'), os.path.join(CSRC, 'w4s_pass_body.inc'), os.path.join(CSRC, 'w4_gemm64h_body.inc'), os.path.join(CSRC, 'w4_wgrad64h_body.inc'), os.path.join(CSRC, 'conv_common.h'), os.path.join(CSRC, 'pointwise_common.h'), os.path.join(CSRC, 'stem.h'), os.path.join(CSRC, 'stem_split.h'), os.path.join(CSRC, 'batchnorm.h'), os.path.join(CSRC, 'bnfunc.h'), os.path.join(CSRC, 'attack.h'), os.path.join(CSRC, 'stem_plan.h'), os.path.join(CSRC, 'ministem.h'), os.path.join(CSRC, 'bnministem.h'), os.path.join(CSRC, 'step_control.h'), os.path.join(CSRC, 'host_common.h'), os.path.join(CSRC, 'butcher.h'),
           os.path.join(CSRC, 'plan.h'), os.path.join(CSRC, 'solver.h'), os.path.join(ROOT, 'include', 'node_hip.h')]
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-Wall', '-Wno-unused-function',
         '-ffp-contract=fast']


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src, diag=False):
    obj = os.path.join(CSRC, src.replace('.hip', '.diag.o' if diag else '.o'))
    path = os.path.join(CSRC, src)
    if _stale(obj, [path] + HEADERS):
        cmd = [HIPCC] + FLAGS + (['-DNODE_DIAG'] if diag else []) + ['-c', path, '-o', obj]
        print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    return obj


def _link(lib, objs, verbose):
    tmp = lib + '.tmp'
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', tmp] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, lib)


def build(force=False, verbose=True, diag=False):
    """Compile every HIP translation unit for gfx950 and link libnode_hip.so (and, with `diag`, libnode_hip_diag.so)."""
    if force:
        for s in SOURCES + [d for d in DIAG_SOURCES if d not in SOURCES]:
            for suffix in ('.o', '.diag.o'):
                o = os.path.join(CSRC, s.replace('.hip', suffix))
                if os.path.exists(o):
                    os.remove(o)
        for lib in (LIB, LIB_DIAG):
            if os.path.exists(lib):
                os.remove(lib)
    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(_compile, SOURCES))
    if _stale(LIB, objs):
        # the guard runs BEFORE the link and a stale library is removed first: a violation never leaves a libnode_hip.so
        # behind that a later, non-forced build() or load would take as up to date
        if os.path.exists(LIB):
            os.remove(LIB)
        _check_asm_loads(verbose)
        _link(LIB, objs, verbose)
    if diag:
        dobjs = [_compile(s, diag=True) if s in DIAG_SOURCES else o for s, o in zip(SOURCES, objs)]
        dobjs += [_compile(s, diag=True) for s in DIAG_SOURCES if s not in SOURCES]
        if _stale(LIB_DIAG, dobjs):
            _link(LIB_DIAG, dobjs, verbose)
    return LIB


def _check_asm_loads(verbose):
    """Before a (re)link: the in-flight-register guard for the kernels with inline-asm loads (tools/check_asm_loads.py,
    which compiles with this module's FLAGS)."""
    tool = os.path.join(os.path.dirname(HERE), 'tools', 'check_asm_loads.py')
    if not os.path.exists(tool):
        return
    r = subprocess.run([sys.executable, tool], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout.strip(), flush=True)
    if r.returncode:
        raise RuntimeError('inline-asm load guard failed:\n' + r.stdout + r.stderr)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, diag='--diag' in sys.argv))
