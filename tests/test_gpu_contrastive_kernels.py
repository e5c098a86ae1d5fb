"""GPU: the contrastive-mode kernels through the C ABI (include/vmc.h) against the float64 references and bounds of
tests/contrastive_refs.py -- vmc_contrastive_prep, vmc_contrastive_softmax, vmc_contrastive_norm_bwd, the workspace functions and the
argument checks.  Every buffer carries guard elements: NaN behind (and between) what a kernel reads, so that a read too far shows in the
output, and a canary bit pattern behind what it writes, compared bit for bit afterwards."""
import ctypes

import numpy as np
import pytest
import torch

import contrastive_refs as R
from contrastive_refs import BF16, DT16, DT_NAME, EPS32, F16, F32, F64, MARGIN

pytestmark = pytest.mark.gpu
E_ARG, E_ALIGN, E_SHAPE, E_DTYPE = -1, -2, -3, -4
CANARY32 = 0x7FC0CA7A                                                                # a NaN with a payload: survives only as bits
CANARY16 = 0x7FC5
GUARD = 64                                                                           # elements; keeps every buffer 16-byte aligned


def _dt(d):
    from vimo_clip_amd import _lib
    return _lib.dt(d)


def _out32(n, dtype=torch.float32):
    """n elements of 4 bytes to be written, canaries everywhere (also behind them)."""
    return torch.full((n + GUARD,), CANARY32, dtype=torch.int32, device="cuda").view(dtype)


def _out16(n, dtype16):
    return torch.full((n + GUARD,), CANARY16, dtype=torch.int16, device="cuda").view(dtype16)


def _tail_intact(buf, n):
    raw = buf.view(torch.int32 if buf.element_size() == 4 else torch.int16)[n:]
    return bool((raw == (CANARY32 if buf.element_size() == 4 else CANARY16)).all().item())


def _untouched(buf):
    return _tail_intact(buf, 0)


def _nan_guarded(x):
    """x (fp32, any shape) flattened on the device with NaN behind it."""
    buf = torch.full((x.numel() + GUARD,), float("nan"), dtype=torch.float32)
    buf[:x.numel()] = x.reshape(-1)
    return buf.cuda()


# ---------------------------------------------------------------------------------------------- prep
def _prep(s, tbuf, rows_per_clip, stride, M, E, dtype16):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    Mp = R.pad64(M)
    u, v, vt, inv = _out16(Mp * E, dtype16), _out16(Mp * E, dtype16), _out16(E * Mp, dtype16), _out32(M)
    check(lib.vmc_contrastive_prep(ptr(s), ptr(tbuf), ptr(u), ptr(v), ptr(vt), ptr(inv), M, E, rows_per_clip, stride, _dt(dtype16),
                                   stream()), "contrastive_prep")
    torch.cuda.synchronize()
    assert _tail_intact(u, Mp * E) and _tail_intact(v, Mp * E) and _tail_intact(vt, E * Mp) and _tail_intact(inv, M)
    return u[:Mp * E].view(Mp, E).cpu(), v[:Mp * E].view(Mp, E).cpu(), vt[:E * Mp].view(E, Mp).cpu(), inv[:M].cpu()


@pytest.mark.parametrize("M,E", [(M, E) for M in R.PREP_M for E in R.PREP_E])
def test_prep_normalises_rounds_pads_and_transposes(M, E):
    s, t = R.prep_inputs(M, E)
    r64, r32 = R.prep_ref(s, t), R.prep_ref(s, t, F32)
    free = ~R.clamp_rows(s)
    for dtype16 in DT16:
        for layout in R.PREP_LAYOUTS:
            tbuf, rpc, stride = R.teacher_buffer(t, layout)
            u, v, vt, inv = _prep(_nan_guarded(s), _nan_guarded(tbuf), rpc, stride, M, E, dtype16)
            tag = f"M {M} E {E} {DT_NAME[dtype16]} {layout}"
            for name, got, key in (("u", u, "u"), ("v", v, "v")):
                x = R.excess16(got[:M], r64[key], R.e32_of(r32[key], r64[key]), dtype16)
                exact = torch.equal(got[:M].view(torch.int16), r64[key].to(F32).to(dtype16).view(torch.int16))
                print(f"{tag}: {name}16 excess {x:.3f}, equals round16(r64) bit for bit: {exact}")
                assert x <= 1.0, (tag, name, x)
                assert exact, (tag, name)                         # the inputs are decided: no element may round the other way
                assert not got[M:].view(torch.int16).any(), (tag, name, "pad rows")
            assert torch.equal(vt.view(torch.int16), v.view(torch.int16).t()), (tag, "transposed copy")
            assert not vt[:, M:].view(torch.int16).any(), (tag, "pad columns")
            if free.any():
                e = R.max_rel(inv[free], r64["inv_s"][free])
                assert e <= R.bound32(R.e32_of(r32["inv_s"][free], r64["inv_s"][free])), (tag, "inv_s", e)
            if (~free).any():
                assert ((inv[~free].double() - 1.0 / R.EPS).abs() <= EPS32 / R.EPS).all(), (tag, "clamped inv_s")


# ---------------------------------------------------------------------------------------------- softmax
def _softmax(z, T, dtype16, want_dz=True, ldz=None):
    """z fp32 [M, M] inside a [M, ldz] buffer whose pad columns and tail hold NaN."""
    from vimo_clip_amd._lib import check, lib, ptr, stream
    M = z.shape[0]
    Mp = R.pad64(M)
    ldz = ldz or Mp + 4
    zb = torch.full((M, ldz), float("nan"))
    zb[:, :M] = z
    zb = _nan_guarded(zb)
    lr, lc, loss, top1 = _out32(M), _out32(M), _out32(1), _out32(1, torch.int32)
    dz = _out16(M * Mp, dtype16)
    nb = lib.vmc_contrastive_partials_bytes(M)
    part = torch.full((nb // 4 + GUARD,), CANARY32, dtype=torch.int32, device="cuda")
    check(lib.vmc_contrastive_softmax(ptr(zb), M, ldz, T, ptr(lr), ptr(lc), ptr(loss), ptr(top1), ptr(dz) if want_dz else None, _dt(dtype16),
                                      ptr(part), nb, stream()), "contrastive_softmax")
    torch.cuda.synchronize()
    assert _tail_intact(lr, M) and _tail_intact(lc, M) and _tail_intact(loss, 1) and _tail_intact(top1, 1) and _tail_intact(part, nb // 4)
    assert _tail_intact(dz, M * Mp) if want_dz else _untouched(dz)
    return {"lse_row": lr[:M].cpu(), "lse_col": lc[:M].cpu(), "loss": loss[:1].cpu(), "top1": int(top1[0]),
            "dz": dz[:M * Mp].view(M, Mp).cpu() if want_dz else None}


@pytest.mark.parametrize("M,T,kind", R.SOFTMAX_CASES)
def test_softmax_statistics_loss_top1_and_gradient(M, T, kind):
    z = R.softmax_inputs(M, kind)
    r64, r32 = R.softmax_ref(z, T), R.softmax_ref(z, T, F32)
    first = None
    for dtype16 in DT16:
        got = _softmax(z, T, dtype16)
        tag = f"M {M} T {T} {kind} {DT_NAME[dtype16]}"
        for k in ("lse_row", "lse_col"):
            e, b = R.max_rel(got[k], r64[k]), R.bound32(R.e32_of(r32[k], r64[k]))
            print(f"{tag}: {k} err {e:.2e} bound {b:.2e}")
            assert e <= b, (tag, k, e, b)
        d, allow = abs(float(got["loss"]) - float(r64["loss"])), R.softmax_loss_allow(r64["loss"], M)
        x = R.dz16_excess(got["dz"][:, :M], r64["dz"], dtype16)
        print(f"{tag}: loss {float(got['loss']):.6g} off by {d:.2e} of {allow:.2e}; dz16 {x:.3f} spacings from round16(r64); top1 {got['top1']}")
        assert d <= allow, (tag, "loss", d, allow)
        assert x <= 1.0, (tag, "dz16", x)
        assert not got["dz"][:, M:].view(torch.int16).any(), (tag, "pad columns")
        assert not got["dz"][:, :M][~r64["valid"]].view(torch.int16).any(), (tag, "masked pairs")
        assert got["top1"] == r64["top1"], (tag, "top1")
        if first is None:
            first = got
        else:                                                      # the fp32 outputs do not depend on the 16-bit type
            assert all(torch.equal(first[k].view(torch.int32), got[k].view(torch.int32)) for k in ("lse_row", "lse_col", "loss"))
    if T == M:                                                     # one clip: only the diagonal is valid
        assert float(first["loss"]) == 0.0 and not first["dz"].view(torch.int16).bitwise_and(0x7FFF).any() and first["top1"] == M


@pytest.mark.parametrize("M,T,kind", [(65, 5, "tau"), (257, 0, "80")])
def test_softmax_without_a_gradient_buffer_and_with_any_leading_dimension(M, T, kind):
    z = R.softmax_inputs(M, kind)
    full = _softmax(z, T, BF16)
    for ldz in (M, M + 1, R.pad64(M) + 64):
        got = _softmax(z, T, BF16, want_dz=False, ldz=ldz)
        assert got["dz"] is None and got["top1"] == full["top1"]
        assert all(torch.equal(full[k].view(torch.int32), got[k].view(torch.int32)) for k in ("lse_row", "lse_col", "loss")), ldz
    again = _softmax(z, T, BF16)
    assert torch.equal(full["dz"].view(torch.int16), again["dz"].view(torch.int16))       # same bits run to run


# ---------------------------------------------------------------------------------------------- norm_bwd
@pytest.mark.parametrize("M,E", R.NORM_BWD_CASES)
def test_norm_bwd_free_rows_and_clamp_rows(M, E):
    from vimo_clip_amd._lib import check, lib, ptr, stream
    s, du = R.norm_bwd_inputs(M, E)
    r64 = R.norm_bwd_ref(du, s)
    e32 = R.e32_of(R.norm_bwd_ref(du, s, F32), r64)
    inv = R.prep_rows(s)[1].to(F32)
    free = ~R.clamp_rows(s)
    out, du_d, s_d, inv_d = _out32(M * E), _nan_guarded(du), _nan_guarded(s), _nan_guarded(inv)
    check(lib.vmc_contrastive_norm_bwd(ptr(du_d), ptr(s_d), ptr(inv_d), ptr(out), M, E, stream()), "contrastive_norm_bwd")
    torch.cuda.synchronize()
    assert _tail_intact(out, M * E)
    got = out[:M * E].view(M, E).cpu()
    for name, rows in (("free", free), ("clamp", ~free)):         # each kind under the plain rule on its own: clamp rows are 1e5 larger
        if rows.any():
            e, b = R.max_rel(got[rows], r64[rows]), R.bound32(R.e32_of(R.norm_bwd_ref(du, s, F32)[rows], r64[rows]))
            print(f"M {M} E {E} {name} rows: err {e:.2e} bound {b:.2e} (all rows e32 {e32:.2e})")
            assert e <= b, (M, E, name, e, b)
    inplace = _nan_guarded(du)                                     # ds may be du itself
    check(lib.vmc_contrastive_norm_bwd(ptr(inplace), ptr(s_d), ptr(inv_d), ptr(inplace), M, E, stream()), "norm_bwd")
    torch.cuda.synchronize()
    assert torch.equal(inplace[:M * E].view(M, E).cpu().view(torch.int32), got.view(torch.int32)) and inplace[M * E:].isnan().all().item()


# ---------------------------------------------------------------------------------------------- workspace and argument checks
def test_workspace_layout_holds_every_part():
    from vimo_clip_amd._lib import lib
    for M, E in ((1, 64), (65, 512), (928, 512), (16384, 768)):
        off = (ctypes.c_size_t * 9)()
        assert lib.vmc_contrastive_workspace_layout(M, E, ctypes.addressof(off)) == 0
        Mp = R.pad64(M)
        need = [Mp * E * 2] * 3 + [M * Mp * 4, M * Mp * 2, M * 4, M * 4, lib.vmc_contrastive_partials_bytes(M)]
        assert off[0] == 0 and all(off[i] % 256 == 0 and off[i + 1] - off[i] >= need[i] for i in range(8))
        assert lib.vmc_contrastive_workspace_bytes(M, E) == off[8] and off[8] <= sum(need) + 8 * 256
    assert 1.5e9 < lib.vmc_contrastive_workspace_bytes(16384, 512) < 1.8e9
    for M, E in ((0, 64), (16385, 64), (4, 96), (4, 0)):
        assert lib.vmc_contrastive_workspace_bytes(M, E) == 0
        assert lib.vmc_contrastive_workspace_layout(M, E, ctypes.addressof((ctypes.c_size_t * 9)())) == E_SHAPE
    assert lib.vmc_contrastive_partials_bytes(0) == 0 and lib.vmc_contrastive_partials_bytes(16385) == 0


def test_argument_and_shape_rejections_return_their_codes_and_write_nothing():
    from vimo_clip_amd._lib import lib, ptr, stream
    M, E = 8, 64
    Mp = R.pad64(M)
    s, t = torch.ones(M * E + GUARD, device="cuda"), torch.ones(M * E + GUARD, device="cuda")
    u, v, vt, inv = _out16(Mp * E, BF16), _out16(Mp * E, BF16), _out16(E * Mp, BF16), _out32(M)

    def prep(s_=s, t_=t, u_=u, v_=v, vt_=vt, inv_=inv, M_=M, E_=E, rpc=M, stride=M * E, d=1):
        return lib.vmc_contrastive_prep(ptr(s_), ptr(t_), ptr(u_), ptr(v_), ptr(vt_), ptr(inv_), M_, E_, rpc, stride, d, stream())
    assert [prep(s_=None), prep(t_=None), prep(u_=None), prep(v_=None), prep(vt_=None), prep(inv_=None)] == [E_ARG] * 6
    assert prep(rpc=0) == E_ARG and prep(rpc=-1) == E_ARG
    assert [prep(M_=0), prep(M_=-3), prep(M_=R.MAX_ROWS + 1), prep(E_=96), prep(E_=0), prep(E_=32)] == [E_SHAPE] * 6
    assert prep(u_=u[1:]) == E_ALIGN and prep(v_=v[4:]) == E_ALIGN and prep(vt_=vt[2:]) == E_ALIGN
    assert prep(d=0) == E_DTYPE and prep(d=3) == E_DTYPE

    z = torch.zeros(M * Mp + GUARD, device="cuda")
    lr, lc, loss, top1, dz = _out32(M), _out32(M), _out32(1), _out32(1, torch.int32), _out16(M * Mp, BF16)
    nb = lib.vmc_contrastive_partials_bytes(M)
    part = torch.full((nb // 4 + GUARD,), CANARY32, dtype=torch.int32, device="cuda")

    def soft(z_=z, M_=M, ldz=Mp, T=2, lr_=lr, lc_=lc, loss_=loss, top1_=top1, dz_=dz, d=1, part_=part, nb_=nb):
        return lib.vmc_contrastive_softmax(ptr(z_), M_, ldz, T, ptr(lr_), ptr(lc_), ptr(loss_), ptr(top1_), ptr(dz_), d, ptr(part_), nb_, stream())
    assert [soft(z_=None), soft(lr_=None), soft(lc_=None), soft(loss_=None), soft(top1_=None), soft(part_=None)] == [E_ARG] * 6
    assert soft(T=-1) == E_ARG and soft(ldz=M - 1) == E_ARG and soft(nb_=nb - 4) == E_ARG
    assert [soft(M_=0), soft(M_=R.MAX_ROWS + 1)] == [E_SHAPE] * 2
    assert soft(d=0) == E_DTYPE and soft(d=7) == E_DTYPE

    ds = _out32(M * E)

    def nbwd(du_=s, s_=t, inv_=s, ds_=ds, M_=M, E_=E):
        return lib.vmc_contrastive_norm_bwd(ptr(du_), ptr(s_), ptr(inv_), ptr(ds_), M_, E_, stream())
    assert [nbwd(du_=None), nbwd(s_=None), nbwd(inv_=None), nbwd(ds_=None)] == [E_ARG] * 4
    assert [nbwd(M_=0), nbwd(M_=R.MAX_ROWS + 1), nbwd(E_=100), nbwd(E_=0)] == [E_SHAPE] * 4
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in (u, v, vt, inv, lr, lc, loss, top1, dz, part, ds))
