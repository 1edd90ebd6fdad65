"""Build-time check of the acquisition kernel for chains with composed-kernel members (csrc/acq_chain_tree.hip; no GPU needed: hipcc
cross-compiles), as test_acq_isa.py and test_acq_stack_tree_isa.py check the other five: every instantiation runs entirely in
registers -- no private (scratch) segment, no vector register spilled -- although it carries the point's coordinates, a running
gradient AND the per-row leaf values through two sweeps, fits a 256-thread workgroup on a CU and takes its LDS dynamically, sized from
the largest member by the host.  Metadata only (the `amdhsa.kernels` block)."""
import pytest

from test_acq_isa import kernels_of

SRC, NAME = "acq_chain_tree.hip", "ffgp_chain_tree_acq_kernel"


@pytest.fixture(scope="module")
def kernels():
    return kernels_of(SRC, NAME)


def test_kernel_has_its_three_instantiations(kernels):
    assert len(kernels) == 3, sorted(kernels)      # D + 1 <= 2, <= 8, <= 16; members and leaf counts are run-time arguments
    # the name keeps clear of the substrings the other five kernels are counted by
    for other in ("ffgp_acq_kernel", "ffgp_stack_acq_kernel", "ffgp_tree_acq_kernel", "ffgp_chain_acq_kernel", "ffgp_stack_tree_acq_kernel"):
        assert not kernels_of(SRC, other), other


def test_kernel_uses_no_scratch(kernels):
    assert kernels
    for name, meta in kernels.items():
        print(name, {k: meta[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count")})
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0, (name, meta)


def test_check_isa_knows_the_source(kernels):
    import check_isa      # (kernels_of has put tools/ on the path)
    sizes = check_isa.check_acq_chain_tree_no_scratch()
    assert len(sizes) == 3 and set(sizes.values()) == {0}


def test_kernel_fits_a_256_thread_workgroup(kernels):
    assert kernels
    for name, meta in kernels.items():
        assert meta["max_flat_workgroup_size"] == 256, (name, meta)
        assert meta["vgpr_count"] <= 512, (name, meta)
        assert meta["group_segment_fixed_size"] == 0, (name, meta)      # dynamic LDS only
