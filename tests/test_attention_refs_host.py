"""CPU: the attention references, error model, selector inputs and case lists of tests/attention_refs.py, without a GPU.

  * attn_ref64 agrees to float64 accuracy with torch's scaled_dot_product_attention under autograd and with the oracle's attention
    (oracle/tfam.py), with masks, and with an autograd softmax under dropout factors;
  * the Python port of attn_route.h that the GPU tests use to assert each case's kernel family equals the header on every case;
  * every case of every list meets the non-vacuity condition (random inputs) and the selector condition (selector inputs), and
    attn_model16 itself passes every criterion;
  * negative controls: wrong attentions in plain torch (a dropped key tile, a mask shifted by one key, a skipped online-softmax
    rescale, delta from the wrong row, no scale in dK, a dropout mask indexed with Tq and Tk swapped) each fail the measure or the
    selector check on at least one case of every family's list that has the mechanism at all."""
import math
import os
import subprocess

import pytest
import torch

import attention_refs as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---------------------------------------------------------------------------------------------- the reference itself
def _autograd(q, k, v, mask, dout, fac, shape, sdpa):
    B, H, Tq, Tk, dh = shape
    qh, kh, vh = (A.heads(t, B, T, H, dh).clone().requires_grad_(True) for t, T in ((q, Tq), (k, Tk), (v, Tk)))
    if sdpa:
        am = None if mask is None else mask[:, None, None, :].expand(B, H, Tq, Tk)
        o = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=am)
    else:
        s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
        if mask is not None:
            s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
        p = torch.softmax(s, -1)
        o = (p if fac is None else p * fac) @ vh
    o.backward(A.heads(dout, B, Tq, H, dh))
    return {"out": A.flat(o.detach()), "dq": A.flat(qh.grad), "dk": A.flat(kh.grad), "dv": A.flat(vh.grad)}


@pytest.mark.parametrize("shape,kind", [((2, 2, 40, 33, 64), "prefix"), ((2, 3, 17, 70, 96), "first16"), ((3, 1, 65, 129, 32), "len1"),
                                        ((2, 2, 5, 7, 8), "none"), ((2, 1, 130, 300, 64), "interior")])
def test_ref64_equals_sdpa_autograd_and_the_oracle(shape, kind):
    B, H, Tq, Tk, dh = shape
    mask = A.make_mask(kind, B, Tk)
    t = A.random_inputs(shape, A.BF16, 5)
    r = A.attn_ref64(t["q"], t["k"], t["v"], mask, t["dout"], shape=shape)
    a = _autograd(t["q"], t["k"], t["v"], mask, t["dout"], None, shape, sdpa=True)
    for n in ("out", "dq", "dk", "dv"):
        assert A.max_rel(a[n], r[n]) <= 1e-12, n
    s = A._scores(A.heads(t["q"], B, Tq, H, dh), A.heads(t["k"], B, Tk, H, dh), mask, dh)
    assert (torch.logsumexp(s, -1) - r["lse"]).abs().max().item() <= 1e-12
    # the oracle's multi-head attention with identity projections (float64, under autograd)
    from oracle import tfam as otfam
    D = H * dh
    eye = torch.eye(D, dtype=F64)
    sd = {"a.in_proj_weight": torch.cat([eye, eye, eye]), "a.in_proj_bias": torch.zeros(3 * D, dtype=F64),
          "a.out_proj.weight": eye, "a.out_proj.bias": torch.zeros(D, dtype=F64)}
    # the oracle projects k and v from one tensor, so it is compared at V = K; the gradient of that tensor is dk + dv
    qi = A.widen(t["q"]).view(B, Tq, D).requires_grad_(True)
    kv = A.widen(t["k"]).view(B, Tk, D).requires_grad_(True)
    o = otfam.mha(sd, "a.", qi, kv, H, key_padding_mask=None if mask is None else ~mask)
    rk = A.attn_ref64(t["q"], t["k"], t["k"], mask, t["dout"], shape=shape)
    assert A.max_rel(o.detach().reshape(B * Tq, D), rk["out"]) <= 1e-12
    o.backward(A.widen(t["dout"]).view(B, Tq, D))
    assert A.max_rel(qi.grad.reshape(B * Tq, D), rk["dq"]) <= 1e-12
    assert A.max_rel(kv.grad.reshape(B * Tk, D), rk["dk"] + rk["dv"]) <= 1e-12


def test_ref64_with_dropout_factors_equals_autograd():
    shape = (2, 2, 40, 70, 64)
    B, H, Tq, Tk, dh = shape
    mask = A.make_mask("first16", B, Tk)
    t = A.random_inputs(shape, A.F16, 6)
    fac = A.dropout_fac(0.25, 99, B, H, Tq, Tk)
    share = (fac == 0).double().mean().item()
    assert abs(share - 0.25) <= 5 * math.sqrt(0.25 * 0.75 / fac.numel())
    assert set(fac.unique().tolist()) == {0.0, float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.25)))}
    assert set(A.dropout_fac(0.5, 1, 1, 1, 8, 8).unique().tolist()) <= {0.0, 2.0}
    r = A.attn_ref64(t["q"], t["k"], t["v"], mask, t["dout"], fac, shape=shape)
    a = _autograd(t["q"], t["k"], t["v"], mask, t["dout"], fac, shape, sdpa=False)
    for n in ("out", "dq", "dk", "dv"):
        assert A.max_rel(a[n], r[n]) <= 1e-12, n


def test_all_masked_clip_is_nan_forward_and_zero_backward():
    shape = (3, 2, 16, 33, 96)
    B, H, Tq, Tk, dh = shape
    mask = A.make_mask("dead", B, Tk)
    t = A.random_inputs(shape, A.BF16, 7)
    r = A.attn_ref64(t["q"], t["k"], t["v"], mask, t["dout"], shape=shape)
    rows = torch.arange(B * Tq) // Tq == 1
    assert torch.isnan(r["out"][rows]).all() and torch.isnan(r["lse"][1]).all()
    assert not torch.isnan(r["out"][~rows]).any()
    krows = torch.arange(B * Tk) // Tk == 1
    assert (r["dq"][rows] == 0).all() and (r["dk"][krows] == 0).all() and (r["dv"][krows] == 0).all()
    assert all(torch.isfinite(r[n]).all() for n in ("dq", "dk", "dv"))


# ---------------------------------------------------------------------------------------------- the route port
def _route_lines():
    lines, want = [], []
    for lst in list(A.MASKED_LISTS.values()) + [A.CAP_CASES]:
        for c in lst:
            B, H, Tq, Tk, dh = A.shape_of(c)
            ld = H * dh + c["pad"]
            lines.append(f"fwd {B} {H} {Tq} {Tk} {dh} {ld} {c['out_off']}")
            want.append(A.route_fwd(Tq, Tk, dh, c["out_off"]))
            lines.append(f"bwd {B} {H} {Tq} {Tk} {dh} {ld} {ld + c['lddq_pad']} {ld} {c['grad_off']} 0")
            want.append("%s %d %d" % A.route_bwd(Tq, Tk, dh, ldd=ld + c["lddq_pad"], ldo=ld, grad_off=c["grad_off"]))
    vit = [(N, N, A.VIT_F, A.VIT_H, 1) for N in A.VIT_N] + [(N, N, A.VIT_LONG_F, A.VIT_LONG_H, 1) for N in A.VIT_LONG_N]
    vit += [(N, 1, A.CLS_F, A.CLS_H, 1) for N in A.CLS_N] + [(A.VARIANT_N, A.VARIANT_N, A.VARIANT_F, A.VARIANT_H, v) for v in A.VARIANTS]
    for N, NQ, F, H, v in vit:
        lines.append(f"vit {N} {NQ} {F} {H} {v}")
        want.append("%s %d %d" % A.route_vit(N, NQ, F, H, v))
    return lines, want


def test_route_port_equals_attn_route_h_on_every_case(tmp_path):
    exe = str(tmp_path / "attn_route_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "attn_route_dump.cpp")])
    lines, want = _route_lines()
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.strip().split("\n")
    assert len(got) == len(want)
    for l, g, w in zip(lines, got, want):
        assert g == w, (l, g, w)


def test_case_lists_name_the_family_they_run_on_and_cover_the_boundaries():
    for name, lst in list(A.MASKED_LISTS.items()) + [("cap", A.CAP_CASES)]:
        ids = [A.case_id(c) for c in lst]
        assert len(set(ids)) == len(ids), name
        for c in lst:
            B, H, Tq, Tk, dh = A.shape_of(c)
            ld = H * dh + c["pad"]
            assert A.route_fwd(Tq, Tk, dh, c["out_off"]) == c["fwd"], A.case_id(c)
            k, block, rs = A.route_bwd(Tq, Tk, dh, ldd=ld + c["lddq_pad"], ldo=ld, grad_off=c["grad_off"])
            assert k == c["bwd"], A.case_id(c)
            if k == A.BM:
                assert (block, rs) == (c["block"], c["rs"]), A.case_id(c)
    fam = {"small": ("fwd", A.SM), "long_fwd": ("fwd", A.LF), "bwd_lds": ("bwd", A.BM), "bwd_tiled": ("bwd", A.LB)}
    for name, (side, k) in fam.items():
        assert all(c[side] == k for c in A.MASKED_LISTS[name]), name
    assert all(A.GF in (c["fwd"],) or c["bwd"] == A.GB for c in A.SCALAR_CASES)
    lds = A.BWD_LDS_CASES + A.SMALL_CASES
    assert {c["block"] for c in lds} == {128, 192, 256}                                   # 2, 3 and 4 waves
    assert {(c["dh"], c["rs"]) for c in lds} == {(64, 144), (64, 128), (96, 208), (96, 192)}   # padded and unpadded rows
    assert any(4 * ((c["Tq"] + 31) & ~31) > 2 * c["block"] for c in lds)                  # the delta remainder loop
    # both sides of the LDS limit, per head dim
    assert A.route_bwd(288, 288, 64)[0] == A.BM and A.route_bwd(289, 289, 64)[0] == A.LB
    assert A.route_bwd(192, 192, 96)[0] == A.BM and A.route_bwd(193, 193, 96)[0] == A.LB
    assert {A.route_vit(N, N, A.VIT_F, A.VIT_H)[1] for N in A.VIT_N} == {0, 5, 6, 7, 8, 9, 10, 11}
    assert all(A.route_vit(N, N, A.VIT_F, A.VIT_H)[1] == A.VIT_INST[N] for N in A.VIT_N)
    assert {A.route_vit(257, 257, A.VARIANT_F, A.VARIANT_H, v)[1] for v in A.VARIANTS} == {1, 2, 3, 4}
    assert all(A.route_vit(257, 257, A.VARIANT_F, A.VARIANT_H, v) == ("ATTN_VIT", A.VARIANT_INST[v], 512 if A.VARIANT_INST[v] in (2, 3) else 520)
               for v in A.VARIANTS)
    assert A.route_vit(257, 1, A.CLS_F, A.CLS_H)[1] == 4
    # every mask kind that kills a leading tile is used, and every masked family has a strided case and a dropout case
    for name, lst in A.MASKED_LISTS.items():
        assert any(c["pad"] for c in lst), name
        assert any(c["drop"] for c in lst), name
    assert {"first16", "last", "len1", "dead"} <= {c["mask"] for c in A.SMALL_CASES}
    assert {"first64", "first128", "last"} <= {c["mask"] for c in A.LONG_FWD_CASES}
    assert {"first64", "interior", "dead"} <= {c["mask"] for c in A.BWD_TILED_CASES}


def test_every_masked_case_runs_with_dropout_but_the_three_whose_clips_all_have_one_live_key():
    every = [c for lst in A.MASKED_LISTS.values() for c in lst]
    assert all(c["drop"] for c in every)
    excluded = [c for c in every if not c["p25"]]
    assert len(excluded) == 3
    for c in excluded:                       # and these still run p = 0.5 on selector inputs
        assert (A.make_mask(c["mask"], c["B"], c["Tk"]).sum(1) == 1).all() if c["mask"] != "none" else c["Tk"] == 1
        assert "sel-p50" in A.ways_of(c) and "rand-p25" not in A.ways_of(c)
    assert all(A.ways_of(c) == A.WAYS for c in every if c["p25"] and c["dh"] > 8)


# ---------------------------------------------------------------------------------------------- every case: conditions, model passes
MASKED = [(name, c) for name, lst in A.MASKED_LISTS.items() for c in lst]


@pytest.mark.parametrize("name,c", MASKED, ids=[f"{n}-{A.case_id(c)}" for n, c in MASKED])
def test_masked_case_meets_the_conditions_and_the_model_passes(name, c):
    for dtype in A.DT16:
        for way in A.ways_of(c):
            P = A.prepare(c, dtype, way)
            r64, model = P["r64"], P["model"]
            if P["sel"]:
                assert A.selector_min_prob(P["t"], P["mask"], P["shape"]) >= A.SEL_PROB
                assert A.selector_loss(P["t"], P["mask"], P["shape"]) <= A.SEL_LOSS
                assert not A.selector_check(model, P["t"], P["mask"], P["shape"], dtype, P["fac"], r64, model)
                pi = P["t"]["pi"]
                live = pi[pi >= 0]
                if c["Tk"] > 64 and c["Tq"] >= 32 and c["mask"] in ("none", "prefix"):          # winners early and late
                    assert (live < 64).any() and (live >= (c["Tk"] - 1) // 64 * 64).any()
            else:                                      # whatever the GPU file holds to the measure (the scalar halves go by e32)
                if A.family_of(c) is not A.FAM_SCALAR:
                    assert not A.vacuity(r64, model, ("out", "lse")), (A.DT_NAME[dtype], way)
                    assert not A.failures(A.measure_all(model, r64, model, ("out", "lse")))
                if A.bwd_family_of(c) is not A.FAM_SCALAR:
                    mb = P.get("model_b", model)
                    assert not A.vacuity(r64, mb, ("dq", "dk", "dv")), (A.DT_NAME[dtype], way)
                    assert not A.failures(A.measure_all(mb, r64, mb, ("dq", "dk", "dv")))


@pytest.mark.parametrize("kind,N", [("vit", N) for N in A.VIT_N] + [("long", N) for N in A.VIT_LONG_N] + [("cls", N) for N in A.CLS_N])
def test_vit_case_meets_the_conditions_and_the_model_passes(kind, N):
    F, H = {"vit": (A.VIT_F, A.VIT_H), "long": (A.VIT_LONG_F, A.VIT_LONG_H), "cls": (A.CLS_F, A.CLS_H)}[kind]
    for dtype in A.DT16:
        P = A.prepare_vit(F, N, H, dtype, "rand", cls=kind == "cls")
        assert not A.vacuity(P["r64"], P["model"], ("out",))
        assert not A.failures(A.measure_all(P["model"], P["r64"], P["model"], ("out", "lse")))
        P = A.prepare_vit(F, N, H, dtype, "sel", cls=kind == "cls")
        assert A.selector_min_prob(P["t"], None, P["shape"]) >= A.SEL_PROB
        assert not A.selector_check(P["model"], P["t"], None, P["shape"], dtype, backward=False)


# ---------------------------------------------------------------------------------------------- negative controls
def _caught(c, dtype, way, bug):
    """Does the wrong attention `bug`, rounding like the model, fail the measure (random inputs) or the selector check?"""
    P = A.prepare(c, dtype, way)
    t, shape = P["t"], P["shape"]
    fac = P["fac"]
    if bug == "dropout_swapped":
        B, H, Tq, Tk, dh = shape
        fac = A.dropout_fac(P["p"], P["seed"], B, H, Tq, Tk, swap=True)
    wrong = A.attn_model16(t["q"], t["k"], t["v"], P["mask"], t["dout"], fac, shape=shape, dtype=dtype, fam=A.family_of(c),
                           bug=None if bug == "dropout_swapped" else bug)
    if P["sel"]:
        return bool(A.selector_check(wrong, t, P["mask"], shape, dtype, P["fac"], P["r64"], P["model"]))
    if A.family_of(c) is A.FAM_SCALAR or A.bwd_family_of(c) is A.FAM_SCALAR:
        r32 = A.attn_ref32(t["q"], t["k"], t["v"], P["mask"], t["dout"], P["fac"], shape=shape)
        return any(A.scalar_excess(n, wrong[n], P["r64"][n], r32[n], dtype) > 1 for n in A.OUTS)
    return bool(A.failures(A.measure_all(wrong, P["r64"], P["model"])))


# attn_small_kernel has one softmax pass over at most 64 keys: no rescale to skip
CONTROLS = [(name, bug) for name in A.MASKED_LISTS for bug in A.BUGS if not (name == "small" and bug == "skip_rescale")]


@pytest.mark.parametrize("name,bug", CONTROLS, ids=[f"{n}-{b}" for n, b in CONTROLS])
def test_negative_control_is_caught_in_every_family(name, bug):
    by_random = by_selector = False
    for c in A.MASKED_LISTS[name]:
        for way in A.ways_of(c):
            if bug == "dropout_swapped" and (way not in A.DROP_P or c["Tq"] == c["Tk"]):
                continue
            hit = _caught(c, A.BF16, way, bug)
            by_selector |= hit and way.startswith("sel")
            by_random |= hit and way.startswith("rand")
        if by_random and by_selector:
            break
    assert by_random, "the measure on random inputs misses it"
    assert by_selector, "the selector check misses it"


@pytest.mark.parametrize("kind", ["vit", "long", "cls"])
@pytest.mark.parametrize("bug", A.FWD_BUGS)
def test_negative_control_is_caught_in_the_vit_families(kind, bug):
    F, H = {"vit": (A.VIT_F, A.VIT_H), "long": (A.VIT_LONG_F, A.VIT_LONG_H), "cls": (A.CLS_F, A.CLS_H)}[kind]
    Ns = {"vit": A.VIT_N, "long": A.VIT_LONG_N, "cls": A.CLS_N}[kind]
    hit = {"rand": False, "sel": False}
    for N in Ns:
        if N < 17:
            continue
        for way in hit:
            P = A.prepare_vit(F, N, H, A.F16, way, cls=kind == "cls")
            wrong = A.vit_forward(P["q"], P["k"], P["v"], P["shape"], A.F16, bug=bug)
            if way == "sel":
                hit[way] |= bool(A.selector_check(wrong, P["t"], None, P["shape"], A.F16, backward=False))
            else:
                hit[way] |= bool(A.failures(A.measure_all(wrong, P["r64"], P["model"], ("out", "lse"))))
        if all(hit.values()):
            break
    assert hit["rand"], "the measure on random inputs misses it"
    # the class query is one row per (frame, head): its single winner need not lie where the bug acts
    assert hit["sel"] or kind == "cls", "the selector check misses it"
