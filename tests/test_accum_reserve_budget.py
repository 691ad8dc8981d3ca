"""Resource budget of the block table's tail kernels beside an accumulation
that runs with a residency reserve (msm_joint.hip "Residency reserve").  CPU
only: the kernel descriptors of the built libkzgx.so (codeobj.py).

A SIMD has 512 VGPRs per lane and the accumulation allocates A of them per
wavefront (BN254: 144, three wavefronts per SIMD).  At reserve 1 a CU holds
one wavefront fewer, so one SIMD holds two and has 512 - 2 A left: stage 1,
stage 2 and the finish must fit in that.  The quotient must fit in the 512 -
3 A that every SIMD has left, as the index pass does.

LDS: a CU has 160 KiB, handed out in granules of 1280 B (measured on the
MI355X: 12 one-wave workgroups per CU up to 12 800 B each, 11 from 12 801 B,
10 from 14 081 B; profiles/accum_reserve_probe.txt).  The reserve asks for
the smallest size under which the occupancy query, which divides 160 KiB by
the byte size, answers one workgroup fewer; the workgroups then hold
ceil(size / 1280) granules each, and stage 2's workgroup must fit in what
they leave.

None of the kernels may carry more scratch than before the reserve existed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "python"))
LIB = os.path.join(ROOT, "kzg-commitments_amd", "libkzgx.so")



@pytest.fixture(autouse=True)
def built():
    assert os.path.exists(LIB), "libkzgx.so is not built"

SIMD_VGPRS = 512
CU_LDS = 160 * 1024
LDS_GRANULE = 1280
# bytes per lane at the commit before the reserve: stage 1 (split), stage 2 (split), finish (split), quotient
SCRATCH_BEFORE = {"BN254": (0, 0, 568, 0), "BLS12381": (0, 0, 892, 0)}
G1 = {"BN254": "7BN254G1", "BLS12381": "10BLS12381G1"}
FR = {"BN254": "7BN254Fr", "BLS12381": "10BLS12381Fr"}


def one(parts):
    import codeobj
    found = codeobj.kernel_resources(LIB, *parts)
    assert len(found) == 1, (parts, sorted(found))
    return next(iter(found.values()))


def kernels(curve):
    g1 = G1[curve]
    accum = one(("13k_joint_accumINS_%sELb0ELb1E" % g1,))  # no entry at infinity, the endomorphism split
    stage1 = one(("15k_joint_horner1INS_%sELb1E" % g1,))
    stage2 = one(("19k_joint_horner2_glvINS_%sELi8E" % g1,))
    stage2_narrow = one(("19k_joint_horner2_glvINS_%sELi4E" % g1,))
    finish = one(("18k_joint_finish_glvINS_%sE" % g1,))
    quotient = one(("17k_quotient_singleINS_%sE" % FR[curve],))
    return accum, stage1, stage2, stage2_narrow, finish, quotient


def lds_left(accum_alloc, r):
    """LDS bytes a CU has left beside the accumulation at reserve r"""
    full = 4 * (SIMD_VGPRS // accum_alloc)
    keep = full - r
    size = CU_LDS // (keep + 1) + 1  # the smallest byte size with CU_LDS // size == keep
    assert CU_LDS // size == keep and CU_LDS // (size - 1) == keep + 1
    held = -(-size // LDS_GRANULE) * LDS_GRANULE
    assert CU_LDS // held == keep  # the hardware admits what the query answered
    return CU_LDS - keep * held


def test_registers_fit_beside_the_reserved_residency():
    accum, stage1, stage2, stage2_narrow, finish, quotient = kernels("BN254")
    assert accum["vgpr_alloc"] == 144 and accum["lds"] == 0 and accum["scratch"] == 0
    room2 = SIMD_VGPRS - 2 * accum["vgpr_alloc"]
    room3 = SIMD_VGPRS - 3 * accum["vgpr_alloc"]
    assert (room2, room3) == (224, 80)
    for k in (stage1, stage2, stage2_narrow, finish):
        assert k["vgpr_alloc"] <= room2, k
    assert quotient["vgpr_alloc"] <= room3, quotient


def test_stage2_lds_fits_beside_the_reserved_residency():
    accum, _, stage2, stage2_narrow, _, _ = kernels("BN254")
    left = lds_left(accum["vgpr_alloc"], 1)
    assert left == 8960  # 128 granules - 11 workgroups x 11 granules
    held = -(-stage2_narrow["lds"] // LDS_GRANULE) * LDS_GRANULE
    assert held <= left, (stage2_narrow, left)
    # the full-wavefront stage 2 (launched without a reserve) would not fit: the reason for the narrow one
    assert -(-stage2["lds"] // LDS_GRANULE) * LDS_GRANULE > left
    assert stage2_narrow["lds"] * 2 == stage2["lds"]
    # two narrow workgroups beside a reserve of 2 as well
    assert held <= lds_left(accum["vgpr_alloc"], 2)


@pytest.mark.parametrize("curve", ["BN254", "BLS12381"])
def test_no_more_scratch_than_before(curve):
    _, stage1, stage2, stage2_narrow, finish, quotient = kernels(curve)
    s1, s2, fin, quo = SCRATCH_BEFORE[curve]
    assert stage1["scratch"] <= s1
    assert stage2["scratch"] <= s2 and stage2_narrow["scratch"] <= s2
    assert finish["scratch"] <= fin
    assert quotient["scratch"] <= quo


def test_descriptors_agree_with_the_symbol_table():
    """the descriptor reader against facts the build states elsewhere: the index pass allocates 48 VGPRs and
    no LDS, stage 2 holds 8 groups x 40 slots x 9 limbs of LDS on BN254"""
    assert one(("13k_joint_indexINS_7BN254G1ELb1E",)) == {"vgpr_alloc": 48, "lds": 0, "scratch": 0}
    assert one(("19k_joint_horner2_glvINS_7BN254G1ELi8E",))["lds"] == 8 * 40 * 9 * 4
