"""Register / scratch budgets of k_dp_cdiv, the forward pass with the two-operation division (k_dp.h), read from
the device ISA the build would produce, the way test_kernel_resources.py holds k_dp<8> and k_dp<5>: the new kernels
must sit on the same occupancy steps as the kernels they replace (128 VGPRs: four wavefronts per SIMD at W = 500;
96: five at W = 300), without scratch.  (No kernel on 217-224 VGPRs: test_kernel_resources.py looks at every kernel
of the build, these included.)"""
import os

import pytest

from test_kernel_resources import _metadata

# kernel name fragment -> max VGPRs (none may use scratch)
BUDGET = {
    '_Z9k_dp_cdivILi8EE': 128,      # W = 500
    '_Z9k_dp_cdivILi5EE': 96,       # W = 300
    '_Z9k_dp_cdivILi4EE': 128,
    '_Z9k_dp_cdivILi12EE': 256,     # start discovery at start_bw = 750
}


@pytest.fixture(scope='module')
def isa_metadata():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    from tombo_amd import _native
    return _metadata(hipcc, [f for f in _native.HIPCC_FLAGS if f not in ('-fPIC', '-shared')])


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_cdiv_kernel_fits_its_occupancy_step(isa_metadata, frag):
    hits = [k for k in isa_metadata if k.startswith(frag)]
    assert len(hits) == 1, (frag, hits)
    m = isa_metadata[hits[0]]
    assert m['vgpr'] <= BUDGET[frag], (hits[0], m)
    assert m['spill'] == 0 and m['scratch'] == 0, (hits[0], m)


def test_every_band_class_has_its_cdiv_kernel(isa_metadata):
    for cpl in (4, 5, 8, 12, 16, 24, 32, 48):
        assert len([k for k in isa_metadata if k.startswith('_Z9k_dp_cdivILi%dEE' % cpl)]) == 1, cpl
