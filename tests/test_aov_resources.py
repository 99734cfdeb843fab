"""The feature-buffer kernels (k_aov, k_aov_bwd) read from the metadata of the BUILT library, like tests/test_kernel_resources.py: they
do the camera ray, first hit and texture lookup of the collocated k_simple kernels without the BRDF, so they must not need more scratch
than those, and their LDS must stay within the 1,280-byte blocks those use.  No GPU needed."""
import re

from test_kernel_resources import LDS_BLOCK, kernels, pick

# mangled template arguments: sampler Li0E (cmj) / Li1E (pmj02bn), accelerator 10BruteAccel / 8BvhAccel
SAMPLERS, ACCELS = ("Li0E", "Li1E"), ("10BruteAccel", "8BvhAccel")
# k_simple<ZDR_COLLOCATED = 0, SK, BruteAccel, BWD, STATS = false, ENV = false, MT = true>: the material-table form the launcher runs
COLLOCATED = r"k_simpleILi0E%s10BruteAccelLb%dELb0ELb0ELb1E"


def blocks(nbytes):
    return -(-nbytes // LDS_BLOCK)


def test_feature_buffer_kernels_exist_for_both_samplers_and_both_accels():
    found = kernels()
    for kernel in ("5k_aov", "9k_aov_bwd"):
        for sk in SAMPLERS:
            for accel in ACCELS:
                assert [n for n in found if re.fullmatch(r"_Z%sI%s%sEv.*" % (kernel, sk, accel), n)], (kernel, sk, accel)


def test_feature_buffer_kernels_need_no_more_scratch_or_lds_than_the_collocated_kernels():
    found = kernels()
    for sk in SAMPLERS:
        for bwd, kernel in ((0, "5k_aov"), (1, "9k_aov_bwd")):
            (name, r), = pick(found, r"_Z%sI%s10BruteAccelEv" % (kernel, sk)).items()
            ref = pick(found, COLLOCATED % (sk, bwd))
            ref_scratch = max(x["private_segment_fixed_size"] for x in ref.values())
            ref_blocks = max(blocks(x["group_segment_fixed_size"]) for x in ref.values())
            print(f"[aov resources] {name}: scratch {r['private_segment_fixed_size']} B (collocated {ref_scratch}), LDS {r['group_segment_fixed_size']} B = "
                  f"{blocks(r['group_segment_fixed_size'])} blocks (collocated {ref_blocks}), {r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs")
            assert r["private_segment_fixed_size"] <= ref_scratch, (name, r, ref)
            assert blocks(r["group_segment_fixed_size"]) <= ref_blocks, (name, r, ref)
