"""GPU: the weight-average kernels through the C ABI (include/vmc.h, K22) -- vmc_ema_update against its float64 reference under the
element bound derived in tests/ema_refs.py, from the step argument and from a device step count, behind the skip flag and chained;
vmc_ema_swap bit for bit; the argument checks.  Every buffer carries 8 guard elements behind n: NaN in the parameters (a read past n
would show in the output), a canary bit pattern in the buffers that are written (compared bit for bit afterwards)."""
import numpy as np
import pytest
import torch

import ema_refs as R

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN = -1, -2
ALL_SIZES = R.SIZES + [R.BIG]
CANARY = 0x7FC0CA7A                                                   # a NaN with a payload: survives only as bits
SPECIAL_BITS = [0x80000000, 0x00000001, 0x807FFFFF, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7FC12345, 0x7F800001, 0xFFFFFFFF, 0x00000000]


def _i32(values):
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32).copy())


def _guarded(x, guard_bits=CANARY):
    """x (numpy fp32 [n]) on the device with GUARD elements of ``guard_bits`` behind it."""
    buf = torch.empty(len(x) + R.GUARD, dtype=torch.float32)
    buf[:len(x)] = torch.from_numpy(np.ascontiguousarray(x))
    buf.view(torch.int32)[len(x):] = _i32([guard_bits] * R.GUARD)
    return buf.cuda()


def _guards_intact(buf, n, guard_bits=CANARY):
    return torch.equal(buf.view(torch.int32)[n:].cpu(), _i32([guard_bits] * R.GUARD))


def _nan_guarded(p):
    buf = torch.full((len(p) + R.GUARD,), float("nan"), dtype=torch.float32)
    buf[:len(p)] = torch.from_numpy(np.ascontiguousarray(p))
    return buf.cuda()


def _update(e_buf, p_buf, n, w, warmup=0, step=0, state=None, skip=None):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    check(lib.vmc_ema_update(ptr(e_buf), ptr(p_buf), n, float(w), int(warmup), int(step), ptr(state), ptr(skip), stream()), "ema_update")
    torch.cuda.synchronize()
    return e_buf[:n].cpu().numpy()


@pytest.mark.parametrize("n", ALL_SIZES)
def test_update_meets_the_element_bound_at_every_size_and_weight(n):
    for i, w in enumerate(R.WEIGHTS):
        e, p = R.inputs(n, seed=i)
        w32 = R.f32v(w)
        e_buf, p_buf = _guarded(e), _nan_guarded(p)
        got = _update(e_buf, p_buf, n, w32)
        x = R.excess(got, e, p, w32)
        print(f"n {n} w {w}: excess {x:.3f} of the element bound")
        assert x <= 1.0, (n, w, x)
        assert _guards_intact(e_buf, n)
        assert not np.array_equal(got, e)


@pytest.mark.parametrize("source", ["argument", "device"])
@pytest.mark.parametrize("t", R.WARMUP_T)
def test_warmup_weight_from_the_step_argument_and_from_device_memory(t, source):
    n = 4101
    omd = R.one_minus_decay(0.9999)
    w = R.weight_of(omd, True, t)
    e, p = R.inputs(n, seed=t % 97)
    e_buf, p_buf = _guarded(e), _nan_guarded(p)
    if source == "argument":
        got = _update(e_buf, p_buf, n, omd, warmup=1, step=t)
    else:
        state = torch.tensor([t, 0x5EED], dtype=torch.int64, device="cuda")
        got = _update(e_buf, p_buf, n, omd, warmup=1, step=0, state=state)      # the argument is ignored when a state is given
        assert state.tolist() == [t, 0x5EED]
    x = R.excess(got, e, p, w)
    print(f"t {t} from {source}: w {float(w):.9g} excess {x:.3f}")
    assert x <= 1.0, (t, source, x)
    assert _guards_intact(e_buf, n)
    # without warm-up the same call uses 1 - decay, whatever the step says
    e_buf = _guarded(e)
    assert R.excess(_update(e_buf, p_buf, n, omd, warmup=0, step=t), e, p, omd) <= 1.0
    if t < 10 ** 5:
        assert R.excess(e_buf[:n].cpu().numpy(), e, p, w) > 1.0           # and the two weights are told apart by the bound


@pytest.mark.parametrize("n", [3, 4101, R.BIG])
def test_skip_flag_leaves_every_byte_even_with_nan_parameters(n):
    e, p = R.inputs(n)
    flag = torch.zeros(2, dtype=torch.int32, device="cuda")
    ref = _update(_guarded(e), _nan_guarded(p), n, 0.5)
    e_buf = _guarded(e)
    assert np.array_equal(_update(e_buf, _nan_guarded(p), n, 0.5, skip=flag).view(np.int32), ref.view(np.int32))      # flag 0 = no flag
    flag[0] = 1
    for warmup, state in ((0, None), (1, torch.tensor([3, 0], dtype=torch.int64, device="cuda"))):
        e_buf = _guarded(e)
        nan_p = torch.full((n + R.GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        got = _update(e_buf, nan_p, n, 0.5, warmup=warmup, state=state, skip=flag)
        assert np.array_equal(got.view(np.int32), e.view(np.int32)) and _guards_intact(e_buf, n)


def test_ten_chained_updates_follow_the_reference_step_by_step():
    n = 4101
    omd = R.one_minus_decay(0.999)
    e0, _ = R.inputs(n, seed=50)
    e_buf = _guarded(e0)
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    prev = e0
    for t in range(1, 11):
        _, p = R.inputs(n, seed=50 + t)
        state[0] = t
        got = _update(e_buf, _nan_guarded(p), n, omd, warmup=1, state=state).copy()
        x = R.excess(got, prev, p, R.weight_of(omd, True, t))             # the reference is fed the kernel's own previous output
        assert x <= 1.0, (t, x)
        prev = got
    assert _guards_intact(e_buf, n)


def test_update_is_one_fused_multiply_add():
    """On the planted inputs of tests/ema_refs.py the fma and the two-rounding `w * d + e` differ in every element: the kernel gives
    the fma's bits (both variants may lie inside the element bound, so the bound cannot tell them apart)."""
    e, p, w = R.planted_two_rounding_input()
    got = _update(_guarded(e), _nan_guarded(p), len(e), w)
    assert np.array_equal(got.view(np.int32), R.ema_model32(e, p, w).view(np.int32))
    assert not (got == R.ema_two_rounding32(e, p, w)).any()


@pytest.mark.parametrize("n", ALL_SIZES)
def test_swap_exchanges_bits_exactly(n):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    rng = np.random.default_rng(n)
    a, b = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    k = min(n, len(SPECIAL_BITS))
    a[:k], b[n - k:] = SPECIAL_BITS[:k], SPECIAL_BITS[::-1][:k]          # -0, subnormals, inf, NaN payloads, at both ends
    a_buf, b_buf = _guarded(a.view(np.float32)), _guarded(b.view(np.float32), CANARY + 1)
    check(lib.vmc_ema_swap(ptr(a_buf), ptr(b_buf), n, stream()), "ema_swap")
    torch.cuda.synchronize()
    assert np.array_equal(a_buf[:n].view(torch.int32).cpu().numpy().view(np.uint32), b)
    assert np.array_equal(b_buf[:n].view(torch.int32).cpu().numpy().view(np.uint32), a)
    assert _guards_intact(a_buf, n) and _guards_intact(b_buf, n, CANARY + 1)
    check(lib.vmc_ema_swap(ptr(a_buf), ptr(b_buf), n, stream()), "ema_swap")          # twice = as it was
    torch.cuda.synchronize()
    assert np.array_equal(a_buf[:n].view(torch.int32).cpu().numpy().view(np.uint32), a)


def test_argument_errors_return_their_codes_and_touch_nothing():
    from vimo_clip_amd._lib import lib, ptr, stream
    n = 64
    e, p = torch.full((n + 8,), 2.0, device="cuda"), torch.full((n + 8,), 3.0, device="cuda")
    state, flag = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

    def upd(e_=e, p_=p, n_=n, w=0.5, warmup=0, step=0, s=None, k=None):
        s = ptr(s) if torch.is_tensor(s) else s
        k = ptr(k) if torch.is_tensor(k) else k
        return lib.vmc_ema_update(ptr(e_), ptr(p_), n_, w, warmup, step, s, k, stream())
    assert upd(e_=None) == E_ARG and upd(p_=None) == E_ARG
    assert upd(w=-1e-3) == E_ARG and upd(w=1.5) == E_ARG and upd(w=float("nan")) == E_ARG
    assert upd(warmup=2) == E_ARG and upd(warmup=-1) == E_ARG and upd(step=-1) == E_ARG
    assert upd(e_=e[1:]) == E_ALIGN and upd(p_=p[1:]) == E_ALIGN
    assert upd(s=state.data_ptr() + 4) == E_ALIGN and upd(k=flag.data_ptr() + 2) == E_ALIGN
    assert upd(e_=e[1:], w=2.0) == E_ARG                                  # the order: argument errors first
    assert upd(n_=0) == 0 and upd(n_=0, e_=e[1:]) == E_ALIGN              # n == 0 is looked at last
    assert upd(w=0.0) == 0 and upd(w=1.0, e_=e[4:], n_=4) == 0            # the closed ends of [0, 1] are accepted

    def swap(a=e, b=p, n_=n):
        return lib.vmc_ema_swap(ptr(a), ptr(b), n_, stream())
    assert swap(a=None) == E_ARG and swap(b=None) == E_ARG and swap(b=e) == E_ARG
    assert swap(b=e[4:], n_=8) == E_ARG and swap(a=e[4:], b=e, n_=8) == E_ARG            # overlapping ranges
    assert swap(a=e[1:]) == E_ALIGN and swap(b=p[1:]) == E_ALIGN
    assert swap(n_=0) == 0 and swap(b=e, n_=0) == E_ARG and swap(a=e[:8], b=e[8:], n_=8) == 0 and swap(a=e[:8], b=e[8:], n_=8) == 0
    torch.cuda.synchronize()
    assert (e[:4] == 2.0).all().item() and (e[8:] == 2.0).all().item() and (e[4:8] == 3.0).all().item()      # only the w = 1 call on e[4:8] wrote
    assert (p == 3.0).all().item() and not state.any().item() and not flag.any().item()
