"""Register budget of the exact-fp32 row-wise kernels (k_rows_linear_f32<false> / <true>), read from the code object inside
libfbbev_hip.so: 256 registers = two waves per SIMD (two 64 KB workgroups per CU), no scratch, no spills.  Pins what the opaque
offset in the LayerNorm epilogue protects: with its bias / LayerNorm pieces hoisted out of the row-tile loop that instantiation
needed 255 registers and 28 bytes of scratch."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_resources as KR  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(os.path.join(KR.LLVM, 'llvm-readelf')) and shutil.which('objcopy')),
                                reason='llvm-readelf / objcopy not available')


def test_both_instantiations_fit_two_waves_per_simd_without_scratch():
    from fb_bev_amd import build
    res = {k: v for k, v in KR.kernel_resources(build.build()).items() if 'k_rows_linear_f32I' in k}
    assert sorted(k.split('k_rows_linear_f32I')[1][:4] for k in res) == ['Lb0E', 'Lb1E'], list(res)
    for k, v in res.items():
        print(k, v)
        assert v['vgpr'] + v.get('agpr', 0) <= 256, (k, v)
        assert v.get('scratch', 0) == 0 and v.get('vgpr_spills', 0) == 0, (k, v)
