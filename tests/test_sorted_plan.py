"""capi.sorted_plan (jfgpu_sorted_plan) on the CPU: what jfgpu_sorted_create will use for a body, computed without a device.
bucket_bits is the smallest B with n_records >> B <= records_per_bucket (0: the default, 8), at most log2(size);
device_bytes is the body, 32 bytes behind it, 8 * (2^B + 1) bytes of index and 2048 bytes of byte tables a key byte."""
import pytest

from jellyfish_amd import capi


def plan(n, lsize, per):
    """The rule restated."""
    per = per or 8
    b = 0
    while (n >> b) > per:
        b += 1
    return min(b, lsize)


@pytest.mark.parametrize("per", [0, 1, 4, 16])
@pytest.mark.parametrize("n", [0, 1, 8, 9, 1 << 20, 1 << 33])
def test_bucket_bits_and_device_bytes(n, per):
    for k, vb in ((21, 4), (100, 1), (128, 8)):
        kb = (2 * k + 7) // 8
        for lsize in (3, 20, 40):                             # below and above the unclamped bucket_bits of the larger n
            bits, nbytes = capi.sorted_plan(n, 1 << lsize, k, vb, per)
            assert bits == plan(n, lsize, per), (n, lsize, per)
            assert nbytes == n * (kb + vb) + 32 + 8 * ((1 << bits) + 1) + 2048 * kb
    assert capi.sorted_plan(9, 1 << 20, 21, 4)[0] == 1 and capi.sorted_plan(8, 1 << 20, 21, 4)[0] == 0
    assert capi.sorted_plan(1 << 33, 1 << 20, 21, 4)[0] == 20 and capi.sorted_plan(1 << 33, 1 << 40, 21, 4)[0] == 30


def test_refusals_need_no_device():
    for args, code in (((10, 1 << 20, 129, 4), capi.E_UNSUPPORTED), ((10, 1 << 20, 21, 9), capi.E_UNSUPPORTED),
                       ((10, 1 << 20, 21, 0), capi.E_INVALID), ((10, 1 << 20, 0, 4), capi.E_INVALID),
                       ((10, (1 << 20) + 1, 21, 4), capi.E_INVALID), ((10, 0, 21, 4), capi.E_INVALID)):
        with pytest.raises(capi.JfgpuError) as e:
            capi.sorted_plan(*args)
        assert e.value.code == code, (args, e.value.msg)
