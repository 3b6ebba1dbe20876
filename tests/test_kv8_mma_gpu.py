"""The matrix-core form of the FP8 KV cache's decode attention (csrc/kernels/kv8.hip attn_decode_q8_mma_kernel; opt-in,
``attn_set_q8_waves(2 / 4)``): the bits of the bf16 matrix-core kernel (v6, same waves per pair) on the dequantised
rows, the exact-answer inputs of tests/kv8_inputs.py, the float reference, max_kv, and the plan's rules."""
from __future__ import annotations

import contextlib

import pytest
import torch

import exact_inputs as xi
import kv8_inputs as k8
import test_kv8_gpu as base  # the shared, cached decode cases and their checks (imported, not edited)
from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DH = xi.DH
B, HKV = 3, 2
SHAPES = [(40, 17), (300, 299), (1030, 700)]


@contextlib.contextmanager
def _mma(waves, rep, t, masked):
    """Pin the matrix-core form at ``waves`` per pair and assert that the plan says so."""
    e = ops.ext()
    try:
        e.attn_reset_knobs()
        e.attn_set_q8_waves(waves)
        rc, why, w, kpg, r = e.attn_decode_q8_plan_check(B, HKV * rep, HKV, DH, t, masked)
        assert rc == 0 and (w, kpg, r) == (waves, 0, rep), (rc, why, w, kpg, r)
        yield e
    finally:
        e.attn_reset_knobs()


def _v6_on_dequantised(q, kq, vq, slot, kvs, mask, waves, max_kv=None):
    e = ops.ext()
    try:
        e.attn_set_v6(2)
        e.attn_set_v6_wpp(waves)
        kd, vd = (k8.to_device(c, "cpu").dequant().to(q.device) for c in (kq, vq))
        return base._attend(q, kd, vd, slot, kvs, mask, max_kv=max_kv)
    finally:
        e.attn_reset_knobs()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", SHAPES)
@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
def test_bits_of_v6_on_the_dequantised_rows(rep, waves, t, slot, masked):
    case = base._decode_case(B, HKV, rep, t, slot, masked)
    q, kq, vq, want = case["random"]
    with _mma(waves, rep, t, masked):
        out = base._attend(q, kq, vq, slot, case["kvs"], case["mask"])
    assert torch.equal(out, _v6_on_dequantised(q, kq, vq, slot, case["kvs"], case["mask"], waves))
    base._close(out, want, 2e-2, 2e-2)  # the float reference on the dequantised rows
    assert float(out[2].abs().max()) == 0  # the row with no valid key


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", SHAPES)
@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("rep", [4, 8])
def test_exact_answers(rep, waves, t, slot, masked):
    case = base._decode_case(B, HKV, rep, t, slot, masked)
    with _mma(waves, rep, t, masked):
        base._check_decode_case(case, B, HKV, rep, slot)  # key census, the three needles, the random case


@pytest.mark.parametrize("waves", [2, 4])
def test_honours_max_kv(waves):
    """t_cap below the slot: the keys from t_cap on are not attended; an unwritten slot (bytes 0, scale 0) inside."""
    rep, t, slot, cap = 4, 300, 299, 150
    case = base._decode_case(B, HKV, rep, t, slot, False)
    q, kq, vq, _ = case["random"]
    kq, vq = (ops.Fp8KV(c.q.clone(), c.scale.clone()) for c in (kq, vq))
    for c in (kq, vq):
        c.q[:, :, 40], c.scale[:, :, 40] = 0, 0
    kvs = case["kvs"].clone()
    kvs[2] = 5
    want = ref.attention(q.cpu(), k8.to_device(kq, "cpu"), k8.to_device(vq, "cpu"), cap - 1, kvs.cpu()).reshape(B, -1)
    with _mma(waves, rep, cap, False):
        out = base._attend(q, kq, vq, slot, kvs, None, max_kv=cap)
    base._close(out, want, 2e-2, 2e-2)
    assert torch.equal(out, _v6_on_dequantised(q, kq, vq, slot, kvs, None, waves, max_kv=cap))


PLAN_LIST = [((2, 32, 8, 64, 100, False), None), ((2, 16, 1, DH, 100, False), None), ((2, 3, 1, DH, 100, False), None),
             ((64, 32, 8, DH, 8192, False), 8), ((255, 32, 8, DH, 384, False), 8), ((256, 32, 8, DH, 384, False), 1),
             ((256, 64, 8, DH, 384, True), 1), ((32, 64, 8, DH, 384, False), 8), ((2048, 8, 1, DH, 384, False), 1)]


def test_plan_rules():
    e = ops.ext()
    e.attn_reset_knobs()
    for args, waves in PLAN_LIST:  # the list of test_kv8_gpu.test_plan_rules: unset, every plan is what it was
        rc, _why, w, kpg, _rep = e.attn_decode_q8_plan_check(*args)
        assert (rc != 0) if waves is None else (rc == 0 and w == waves and kpg > 0), (args, rc, w, kpg)
    try:
        for waves in (2, 4):
            e.attn_set_q8_waves(waves)
            assert e.attn_decode_q8_plan_check(2, 16, 1, DH, 100, False)[0] != 0   # rep 16 stays refused
            for args in ((1, 32, 8, DH, 8192, False), (256, 64, 8, DH, 384, True)):  # (the first splits by default)
                assert e.attn_decode_q8_plan_check(*args)[:4] == (0, "", waves, 0)
                assert e.attn_decode_q8_split_check(*args) == (0, "", 1, 0, 0)
            e.attn_set_q8_splits(4)
            assert e.attn_decode_q8_plan_check(1, 32, 8, DH, 8192, False)[0] != 0  # no key splits in this form
            e.attn_set_q8_splits(0)
        e.attn_set_q8_waves(3)  # not a form: by shape
        assert e.attn_decode_q8_plan_check(32, 64, 8, DH, 384, False)[2] == 8
    finally:
        e.attn_reset_knobs()
