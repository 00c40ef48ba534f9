"""The 29-bit-limb field layer (csrc/field29.h) on the device, one primitive
per launch through qg_selftest_field29, at the operand edges its contract
documents (tests/field29_vectors.py): the gfx950 build of the QG_HD forms
against Python integers and limb for limb against the host build, and the
device-only throughput forms (mul29t, sqr29t, mulsub29t, mul29t2, sqr29t2,
mul29tn<3>, <4>) against Python integers, the plain forms and each other."""
import pytest

import field29_vectors as fv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd(dev):
    """device results of the host-callable product ops, per field (each case
    asserted against the Python reference on the way)"""
    return {field: fv.check_field_hd(dev.h, field, 1) for field in (0, 1)}


@pytest.mark.parametrize("field", [0, 1], ids=["Fr", "Fq"])
def test_hd_primitives_on_device(hd, field):
    host = fv.check_field_hd(None, field, 0)
    for op in ("MUL", "SQR", "MULSUB"):
        assert hd[field][op] == host[op], op  # the same limbs from both builds


@pytest.mark.parametrize("field", [0, 1], ids=["Fr", "Fq"])
def test_throughput_forms(dev, hd, field):
    fv.check_field_device_only(dev.h, field, hd[field])


def test_partial_wave_and_empty_launch(dev):
    """n that is no multiple of the block, n = 1 and n = 0"""
    p = fv.P_MOD
    mc = fv.mul_cases(p).kept
    for n in (0, 1, 63, 65):
        res = fv.run_field(dev.h, 1, fv.F29["MULT"], 1, [(a.l, b.l) for a, b in mc[:n]])
        assert len(res) == n
        for (a, b), r in zip(mc, res):
            fv.check_mul(p, a, b, r[0], "mul29t")
