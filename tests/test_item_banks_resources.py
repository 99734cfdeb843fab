"""The private segment of the backward path kernels, read from the metadata of the BUILT library (no GPU needed; the reader is
tests/test_kernel_resources.py's).

k_path_bwd's private memory is meant to hold the overflow records of the pool and nothing else: deep_link[16] (64 bytes) and
deep[16] (16 x 80 bytes), 1,344 bytes, which the compiler rounds to 1,360.  The parent of the change that added this file had
16 bytes more in every instantiation: the item banks' bookkeeping (ItemBanks: two small arrays indexed by the wave-uniform
bank) was demoted to scratch memory and read and written through the vector-memory path on every trip of the persistent loop
(profiles/item_banks_isa.txt).  As four named scalars it lives in SGPRs."""
import re

from test_kernel_resources import kernels, pick

# private_segment_fixed_size of every k_path_bwd instantiation in the PARENT of that change (dcb46b0), by template arguments
# <sampler, accel, ENV, MT, EG, LG>: a table of what was, not a wish — no instantiation may need more than it did.
PARENT_PRIVATE_SEGMENT = {
    (0, "brute", 0, 0, 0, 0): 1376, (0, "brute", 0, 1, 0, 0): 1376, (0, "brute", 0, 1, 0, 1): 1376,
    (0, "brute", 1, 0, 0, 0): 1392, (0, "brute", 1, 1, 0, 0): 1392, (0, "brute", 1, 1, 0, 1): 1376, (0, "brute", 1, 1, 1, 0): 1440,
    (0, "bvh", 0, 0, 0, 0): 1920, (0, "bvh", 0, 1, 0, 0): 1936, (0, "bvh", 0, 1, 0, 1): 1696,
    (0, "bvh", 1, 0, 0, 0): 1920, (0, "bvh", 1, 1, 0, 0): 1936, (0, "bvh", 1, 1, 0, 1): 1696, (0, "bvh", 1, 1, 1, 0): 1984,
    (1, "brute", 0, 0, 0, 0): 1376, (1, "brute", 0, 1, 0, 0): 1376, (1, "brute", 0, 1, 0, 1): 1376,
    (1, "brute", 1, 0, 0, 0): 1376, (1, "brute", 1, 1, 0, 0): 1376, (1, "brute", 1, 1, 0, 1): 1376, (1, "brute", 1, 1, 1, 0): 1424,
    (1, "bvh", 0, 0, 0, 0): 1904, (1, "bvh", 0, 1, 0, 0): 1936, (1, "bvh", 0, 1, 0, 1): 1680,
    (1, "bvh", 1, 0, 0, 0): 1904, (1, "bvh", 1, 1, 0, 0): 1904, (1, "bvh", 1, 1, 0, 1): 1680, (1, "bvh", 1, 1, 1, 0): 1968,
}
NAME = re.compile(r"^_Z10k_path_bwdILi([01])E(10BruteAccel|8BvhAccel)Lb([01])ELb([01])ELb([01])ELb([01])EE")


def backward_kernels():
    found = {}
    for name, r in pick(kernels(), r"^_Z10k_path_bwdI").items():
        m = NAME.match(name)
        assert m, name
        key = (int(m.group(1)), "brute" if "Brute" in m.group(2) else "bvh", *(int(m.group(i)) for i in (3, 4, 5, 6)))
        found[key] = r
    return found


def test_brute_force_backward_kernels_hold_the_overflow_records_only():
    """k_path_bwd<*, BruteAccel, ENV = false, ...>: 16 links + 16 records = 1,344 bytes, 1,360 with the rounding, and not a byte
    for the item banks (all six sat at 1,376)."""
    sel = {k: r for k, r in backward_kernels().items() if k[1] == "brute" and k[2] == 0}
    assert len(sel) == 6, sorted(sel)
    for k, r in sel.items():
        assert r["private_segment_fixed_size"] <= 1360, (k, r)


def test_no_backward_kernel_has_a_larger_private_segment_than_in_the_parent():
    found = backward_kernels()
    assert sorted(found) == sorted(PARENT_PRIVATE_SEGMENT), sorted(set(found) ^ set(PARENT_PRIVATE_SEGMENT))
    for k, r in found.items():
        assert r["private_segment_fixed_size"] <= PARENT_PRIVATE_SEGMENT[k], (k, r, PARENT_PRIVATE_SEGMENT[k])
