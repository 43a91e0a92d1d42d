"""The residual-block unit ships only the kernels its dispatcher can launch: one row per step at C = 64, two rows per step at
C = 128, each for bf16 and IEEE half (the variants NOTES.md measured and closed are not built), and none of the first-stage
row walkers uses scratch."""
import os
import re
import shutil
import subprocess

import pytest

from test_isa_lint import _device_code_objects, LLVM
from yolo_amd import lib as L

RES_BLOCK_KERNELS = {'res_block_kernel<64, bf16_t>', 'res_block_kernel<64, f16_t>', 'res_block2_kernel<128, bf16_t>', 'res_block2_kernel<128, f16_t>'}


def test_res_block_kernel_set_and_no_scratch_in_the_row_walkers(tmp_path):
    if not os.path.exists(os.path.join(LLVM, 'llvm-readelf')) or not shutil.which('make') or not shutil.which('c++filt'):
        pytest.skip('no ROCm LLVM tools here')
    L.build()
    scratch = {}
    for co in _device_code_objects(os.path.join(L.CSRC, 'libyolo_amd.so'), str(tmp_path)):
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], capture_output=True, text=True, check=True).stdout
        fields = [dict(re.findall(r'\.(\w+):\s+(\S+)', '.agpr_count:' + b.split('\n    - .a')[0])) for b in notes.split('- .agpr_count:')[1:]]
        dem = subprocess.run(['c++filt'], input='\n'.join(f.get('name', '?') for f in fields), capture_output=True, text=True).stdout.split('\n')
        for f, d in zip(fields, dem):
            m = re.match(r'void ((?:res_block2?|stem_down|stem_res)_kernel<[^>]*>)\(', d)
            if m:
                scratch[m.group(1)] = int(f.get('private_segment_fixed_size', -1))
            else:
                assert 'res_block' not in d, 'a kernel of the residual-block unit with an unexpected signature: %s' % d
    assert {k for k in scratch if 'res_block' in k} == RES_BLOCK_KERNELS
    assert {k for k in scratch if 'res_block' not in k} == {'stem_down_kernel<bf16_t>', 'stem_down_kernel<f16_t>', 'stem_res_kernel<bf16_t>', 'stem_res_kernel<f16_t>'}
    assert not {k: s for k, s in scratch.items() if s != 0}, 'row walkers with scratch (an unroll failure or a register cliff)'
