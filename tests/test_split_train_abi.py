"""CPU checks of the split training path's C ABI (revision 5): the new entries are declared in include/yolo_amd.h and bound in
yolo_amd.lib.SIGNATURES, the revisions agree, and the split training kernels of the built library keep no scratch and issue no
scalar-memory instruction other than a load."""
import os
import re
import shutil
import subprocess

import pytest

from yolo_amd import lib as L
from test_isa_lint import LLVM, _device_code_objects

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'yolo_amd.h')
NEW = ('yolo_conv_wgrad_split', 'yolo_conv_wgrad_split_workspace_bytes', 'yolo_add_split')


def test_split_training_entries_declared_and_bound():
    h = open(HEADER).read()
    assert int(re.search(r'#define YOLO_ABI_VERSION (\d+)', h).group(1)) == L.ABI_VERSION == 5
    for name in NEW:
        assert re.search(r'\b%s\(' % name, h), name
        assert name in L.SIGNATURES, name
        # the argument count of the binding matches the header's prototype
        proto = re.search(r'(?:int|long long) %s\(([^)]*)\)' % name, h).group(1)
        assert len(proto.split(',')) == len(L.SIGNATURES[name][1]), name


SPLIT_KERNELS = [r'wgrad_split_kernel<1, 1>', r'wgrad_split_kernel<2, 2>', r'bn_reduce_kernel<bf16x3_t, 0>',
                 r'bn_reduce_kernel<bf16x3_t, 1>', r'bn_apply_kernel<bf16x3_t, 0, 1>', r'bn_apply_kernel<bf16x3_t, 1, 1>',
                 r'bias_grad_kernel<bf16x3_t>', r'gather_rows_kernel<bf16x3_t>', r'dilate2_kernel<bf16x3_t>', r'upcat_bwd_kernel<bf16x3_t>',
                 r'add_kernel<bf16x3_t>', r'upsample_concat_kernel<2>', r'nchw_to_nhwc_kernel<bf16x3_t, 8>']


def test_split_training_kernels_have_no_scratch(tmp_path):
    readelf = os.path.join(LLVM, 'llvm-readelf')
    if not os.path.exists(readelf) or not shutil.which('make') or not shutil.which('c++filt'):
        pytest.skip('no ROCm LLVM tools here')
    L.build()
    so = os.path.join(L.CSRC, 'libyolo_amd.so')
    found = {}
    for co in _device_code_objects(so, str(tmp_path)):
        notes = subprocess.run([readelf, '--notes', co], capture_output=True, text=True, check=True).stdout
        blocks = notes.split('- .agpr_count:')[1:]
        names = [dict(re.findall(r'\.(\w+):\s+(\S+)', '.agpr_count:' + b.split('\n    - .a')[0])) for b in blocks]
        dem = subprocess.run(['c++filt'], input='\n'.join(f.get('name', '?') for f in names), capture_output=True, text=True).stdout.split('\n')
        for f, d in zip(names, dem):
            for pat in SPLIT_KERNELS:
                if pat in d:
                    found.setdefault(pat, []).append((d, int(f.get('private_segment_fixed_size', -1))))
    missing = [p for p in SPLIT_KERNELS if p not in found]
    assert not missing, 'split training kernels not in the library: %s' % missing
    spilled = [(d, s) for v in found.values() for d, s in v if s != 0]
    assert not spilled, 'split training kernels with scratch: %s' % spilled


# The scalar-memory (SMEM) encoding of gfx9-family code: the first dword's bits [31:26] are 0b110000.  The only SMEM instructions the
# split training kernels may contain are loads of their arguments / constants, the cache invalidation and the clock reads.
SMEM_ALLOWED = ('s_load_', 's_buffer_load_', 's_dcache_inv', 's_memtime', 's_memrealtime')


def test_split_training_kernels_scalar_memory_is_loads_only(tmp_path):
    objdump = os.path.join(LLVM, 'llvm-objdump')
    if not os.path.exists(objdump) or not shutil.which('make') or not shutil.which('c++filt'):
        pytest.skip('no ROCm LLVM tools here')
    L.build()
    so = os.path.join(L.CSRC, 'libyolo_amd.so')
    seen, smem, other = set(), 0, []
    for co in _device_code_objects(so, str(tmp_path)):
        dis = subprocess.run([objdump, '-d', '--demangle', '--mcpu=gfx950', co], capture_output=True, text=True, check=True).stdout
        for sym in re.split(r'\n(?=[0-9a-f]+ <)', dis):
            m = re.match(r'[0-9a-f]+ <(.*)>:\s*$', sym.split('\n', 1)[0])           # (template names hold '<' and '>')
            hit = [p for p in SPLIT_KERNELS if m and p in m.group(1)]
            if not hit:
                continue
            seen.update(hit)
            for ln in sym.split('\n'):
                e = re.search(r'//\s*[0-9A-Fa-f]+:\s*([0-9A-Fa-f]{8})', ln)
                if e and (int(e.group(1), 16) >> 26) == 0b110000:
                    smem += 1
                    if not ln.strip().startswith(SMEM_ALLOWED):
                        other.append(ln.strip())
    assert set(SPLIT_KERNELS) <= seen, 'split training kernels not found in the disassembly: %s' % sorted(set(SPLIT_KERNELS) - seen)
    assert smem > 0, 'no scalar-memory instruction recognised: the encoding column of the disassembly changed?'
    assert not other, other[:5]
