"""CPU tier (hipcc cross-compiles without a GPU): the register budget of ALL four paired chain kernels of nero_amd/csrc/mlp_f16p.hip.

tests/test_no_packed_fp32.py pins fwd_p_kernel and tan_p_kernel; DESIGN.md 9.2 says both bwd_p_kernel instances are spill-free too, and
nothing pinned that.  The kernels only pay while two workgroups share a CU (256 threads each = two waves per SIMD = at most 256 VGPRs per
wave), and a spilled register is a scratch access that waits on vmcnt -- in kernels whose waits are counted by hand (mlp_f16_util.h:
gemm_f16x3_dual_fixed) a compiler-inserted scratch reload would also drain the weight ring and the row stores."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags():
    src = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    m = re.search(r"flags = \[([^\]]*)\]", src)
    return [f.strip().strip("'") for f in m.group(1).split(',')]


def _kernel_metadata():
    path = os.path.join(ROOT, 'nero_amd', 'csrc', 'mlp_f16p.hip')
    p = subprocess.run(['hipcc'] + _flags() + ['-S', '--cuda-device-only', '-o', '-', path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    meta = {}
    text = p.stdout[p.stdout.index('amdhsa.kernels:'):]
    for entry in re.split(r'\n  - ', text)[1:]:          # one YAML list item per kernel
        nm = re.search(r'\.name:\s+(\S+)', entry)
        if nm is None:
            continue
        meta[nm.group(1)] = {m.group(1): int(m.group(2)) for m in
                             re.finditer(r'\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)', entry)}
    return meta


def test_every_paired_kernel_fits_two_workgroups_per_cu_without_scratch():
    meta = _kernel_metadata()
    wanted = {'fwd_p_kernelE': 1, 'tan_p_kernelE': 1, 'bwd_p_kernelILb1EE': 1, 'bwd_p_kernelILb0EE': 1}
    for key, count in wanted.items():
        hit = {n: v for n, v in meta.items() if key in n}
        assert len(hit) == count, (key, sorted(meta))
        for name, v in hit.items():
            assert v['max_flat_workgroup_size'] == 256, (name, v)
            assert v['vgpr_count'] <= 256, (name, v)
            assert v['vgpr_spill_count'] == 0, (name, v)
            assert v['private_segment_fixed_size'] == 0, (name, v)
    assert len(meta) == 4, sorted(meta)                   # no further instance of a paired kernel
