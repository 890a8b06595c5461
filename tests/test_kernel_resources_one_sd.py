"""Register / scratch budgets of k_dp_c1, the forward pass of a model with one proven sd (k_dp.h), read from the
device ISA the build would produce, the way test_kernel_resources.py and test_dp_cdiv_resources.py hold the kernels it
stands in for: the 8-cell class on 128 VGPRs (four wavefronts per SIMD at W = 500), the 12-cell class of start
discovery on no more than the 196 its k_dp_cdiv build has, none with scratch, none on the 217-224 registers
test_kernel_resources.py forbids for every kernel of the build."""
import os

import pytest

from test_kernel_resources import _metadata

# kernel name fragment -> max VGPRs (none may use scratch)
BUDGET = {
    '_Z7k_dp_c1ILi8EE': 128,        # W = 500
    '_Z7k_dp_c1ILi12EE': 196,       # start discovery at start_bw = 750
    '_Z7k_dp_c1ILi5EE': 96,         # W = 300
    '_Z7k_dp_c1ILi4EE': 128,
}


@pytest.fixture(scope='module')
def isa_metadata():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    from tombo_amd import _native
    return _metadata(hipcc, [f for f in _native.HIPCC_FLAGS if f not in ('-fPIC', '-shared')])


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_one_sd_kernel_fits_its_occupancy_step(isa_metadata, frag):
    hits = [k for k in isa_metadata if k.startswith(frag)]
    assert len(hits) == 1, (frag, hits)
    m = isa_metadata[hits[0]]
    assert m['vgpr'] <= BUDGET[frag], (hits[0], m)
    assert m['spill'] == 0 and m['scratch'] == 0, (hits[0], m)


def test_every_band_class_has_its_one_sd_kernel_and_none_sits_on_224_vgprs(isa_metadata):
    for cpl in (4, 5, 8, 12, 16, 24, 32, 48):
        hits = [k for k in isa_metadata if k.startswith('_Z7k_dp_c1ILi%dEE' % cpl)]
        assert len(hits) == 1, cpl
        assert (isa_metadata[hits[0]]['vgpr'] + 7) // 8 != 28, (hits[0], isa_metadata[hits[0]])
