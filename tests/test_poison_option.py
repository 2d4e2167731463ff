"""CPU test of the POISON option's argument handling (komb_set_option; the fill itself runs in tests/test_gpu_dirty_memory.py):
a 32-bit word in any base strtoull reads is accepted, anything else is refused with KOMB_ERR_ARG and a message that names
the option, and NULL (which unsets it) is accepted whether it is set or not.  Options are per-context host state: no device
is needed to set them."""
import pytest

VALID = ["0xFFFFFFFF", "0x7FFFFFFF", "0x00000001", "0x80000000", "0", "4294967295", "0XA5A5A5A5"]
MALFORMED = ["", "junk", "0x1FFFFFFFF", "4294967296", "0xFFFFFFFF ", "12abc", "-"]


def test_poison_option_values(built):
    import komb_amd
    from komb_amd import _lib
    with komb_amd.KombAccel() as a:
        for v in VALID:
            a.set_option("POISON", v)
        for v in MALFORMED:
            with pytest.raises(komb_amd.KombError) as e:
                a.set_option("POISON", v)
            assert e.value.code == _lib.KOMB_ERR_ARG, v
            assert "POISON" in a._lib.komb_last_error(a._ctx).decode(), v
        a.set_option("POISON", None)                 # NULL unsets ...
        a.set_option("POISON", None)                 # ... and unsetting an unset option is no error
        a.set_option("POISON", "0x80000000")
