"""CPU tests of the allocation-failure hook's host side (komb_set_option ALLOC_FAIL_AT / ALLOC_TRIM_AT, komb_alloc_info; the
injected failures themselves run in tests/test_gpu_alloc_failure.py): a non-negative decimal request number is accepted,
anything else is refused with KOMB_ERR_ARG and a message that names the option and changes nothing, NULL disarms whether or
not the option is set, komb_alloc_info answers on a context without a device, and neither option is among the names the test
plumbing forwards from the environment (forwarding would re-arm a one-shot trigger before every call)."""
import ctypes

import pytest

NAMES = ["ALLOC_FAIL_AT", "ALLOC_TRIM_AT"]
VALID = ["0", "1", "7", "420", "9223372036854775807", "007"]
MALFORMED = ["", "junk", "-1", "+1", " 1", "1 ", "0x10", "1.5", "12abc", "9223372036854775808", "-"]
FIELDS = ("requests", "fired", "pool_blocks_in_use", "pool_bytes_in_use", "pool_blocks_cached", "trims")


@pytest.mark.parametrize("name", NAMES)
def test_alloc_option_values(built, name):
    import komb_amd
    from komb_amd import _lib
    with komb_amd.KombAccel() as a:
        for v in VALID:
            a.set_option(name, v)
        for v in MALFORMED:
            with pytest.raises(komb_amd.KombError) as e:
                a.set_option(name, v)
            assert e.value.code == _lib.KOMB_ERR_ARG, v
            assert name in a._lib.komb_last_error(a._ctx).decode(), v
        a.set_option(name, None)                     # NULL disarms ...
        a.set_option(name, None)                     # ... and disarming an unset option is no error
        a.set_option(name, "3")
        assert a.alloc_info() == dict.fromkeys(FIELDS, 0)   # armed, and nothing has asked for memory


def test_alloc_info_without_a_device(built):
    """Host state only: every field is readable on a context whatever its device, any output may be NULL, a NULL context is
    KOMB_ERR_ARG."""
    import komb_amd
    from komb_amd import _lib
    lib = _lib.load()
    assert lib.komb_alloc_info(None, None, None, None, None, None, None) == _lib.KOMB_ERR_ARG
    with komb_amd.KombAccel(flags=_lib.KOMB_CREATE_NO_WARMUP) as a:
        assert a.alloc_info() == dict.fromkeys(FIELDS, 0)
        assert lib.komb_alloc_info(a._ctx, None, None, None, None, None, None) == 0
        req, fired = ctypes.c_int64(-7), ctypes.c_int32(-7)
        assert lib.komb_alloc_info(a._ctx, ctypes.byref(req), ctypes.byref(fired), None, None, None, None) == 0
        assert (req.value, fired.value) == (0, 0)
        a.set_option("ALLOC_FAIL_AT", "1")
        a.set_option("ALLOC_FAIL_AT", None)
        assert a.alloc_info() == dict.fromkeys(FIELDS, 0)


def test_a_refused_value_changes_nothing(built):
    import komb_amd
    with komb_amd.KombAccel() as a:
        a.set_option("ALLOC_FAIL_AT", "5")
        with pytest.raises(komb_amd.KombError):
            a.set_option("ALLOC_FAIL_AT", "five")
        with pytest.raises(komb_amd.KombError):
            a.set_option("ALLOC_TRIM_AT", "-2")
        assert a.alloc_info() == dict.fromkeys(FIELDS, 0)


def test_alloc_options_are_not_forwarded_from_the_environment(built):
    import komb_amd.api
    for name in NAMES:
        assert name not in komb_amd.api.OPTION_NAMES
