"""Host: the paired launch of an augmented evaluation's weight gradient and conv-1 data gradient (k_w4_gemm64h_wgrad64h,
csrc/kernels_w4_wgrad.hip) is in the library, and the compiler gave every instantiation its registers without scratch.

The kernel is two stand-alone kernels' bodies behind one branch and is allocated for the larger of them: a spill would put scratch
traffic into two memory-bound loops.  The test builds the library, looks the kernel's name up in it, then compiles the file for
gfx950 (no GPU needed) and reads the compiler's resource remarks.  The default variant <D = 2, MINB = 2> must also keep the two
workgroups per CU that k_w4_wgrad64h has on its own: at most 256 registers."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = 'k_w4_gemm64h_wgrad64h'


def _build_module():
    spec = importlib.util.spec_from_file_location('node_amd_build', os.path.join(ROOT, 'neural-ode-features_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_paired_kernel_is_in_the_library():
    b = _build_module()
    lib = b.build(verbose=False)
    blob = open(lib, 'rb').read()
    for inst in ('ILi4ELi1EE', 'ILi2ELi1EE', 'ILi2ELi2EE'):      # <D, MINB>: the mangled names the host registers the kernels under
        assert ('_ZN4node21%s%s' % (KERNEL, inst)).encode() in blob, inst


def test_paired_kernel_uses_no_scratch(tmp_path):
    b = _build_module()
    asm = str(tmp_path / 'kernels_w4_wgrad.s')
    r = subprocess.run([b.HIPCC] + b.FLAGS + ['--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage',
                                              os.path.join(b.CSRC, 'kernels_w4_wgrad.hip'), '-o', asm], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got, cur = {}, None
    for line in r.stderr.split('\n'):
        m = re.search(r'remark:\s+Function Name: (\S+)', line)
        if m:
            cur = got.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    pairs = {k: v for k, v in got.items() if KERNEL in k}
    print(pairs)
    assert len(pairs) == 3, sorted(got)
    for name, res in pairs.items():
        assert res['ScratchSize'] == 0, (name, res)
    dflt = pairs['_ZN4node21%sILi2ELi2EEEvNS_10W4PairArgsE' % KERNEL]
    assert dflt['VGPRs'] + dflt['AGPRs'] <= 256 and dflt['Occupancy'] >= 2, dflt
    # the stand-alone weight gradient keeps what it had: no scratch, two workgroups per CU
    alone = got['_ZN4node13k_w4_wgrad64hENS_12W4WgradHArgsE']
    assert alone['ScratchSize'] == 0 and alone['Occupancy'] >= 2, alone
