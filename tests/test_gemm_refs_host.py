"""CPU: the references, case lists and measure of tests/gemm_refs.py, which tests/test_gpu_gemm_parity.py holds the GEMM kernels to.

  * linear_ref64 against torch.nn.functional.linear + torch's activations in float64, and its row maps on a hand-made example;
  * every case through tests/host/gemm_route_dump.cpp (gemm_route.h itself): the plan it is named for, and the union of the lists
    covers every routed kernel;
  * per case: e32 <= E32_MAX and, for 16-bit outputs, the share of elements the interval rule pins to the bit;
  * the measure itself: a float32 CPU evaluation with round-to-nearest stores passes every case, and each of eight mutants of that
    evaluation fails the case named for it."""
import os
import subprocess

import pytest
import torch

import gemm_refs as G
from gemm_refs import BF16, F16, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    G.clear()


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_linear_ref64_matches_torch(act):
    g = torch.Generator().manual_seed(act)
    a, w = torch.randn(37, 64, generator=g, dtype=F64), torch.randn(20, 64, generator=g, dtype=F64)
    b, res = torch.randn(20, generator=g, dtype=F64), torch.randn(37, 20, generator=g, dtype=F64)
    z = torch.nn.functional.linear(a, w, b)
    y = (z, z * torch.sigmoid(1.702 * z), torch.nn.functional.gelu(z), torch.relu(z))[act]
    r = G.linear_ref64(a, w, bias=b, res=res, act=act, alpha=0.75)
    assert (r["Z"] - z).abs().max().item() <= 1e-12
    assert (r["C"] - (0.75 * y + res)).abs().max().item() <= 1e-12
    assert (G.linear_ref64(a, w)["C"] - a @ w.t()).abs().max().item() <= 1e-12


def test_row_maps_by_hand():
    # two frames of three patches: token rows 1 2 3 | 5 6 7 (0 and 4 are the class rows), positional rows 0 1 2 | 0 1 2
    orow, rrow = G.row_maps(6, 3, 3)
    assert orow.tolist() == [1, 2, 3, 5, 6, 7] and rrow.tolist() == [0, 1, 2, 0, 1, 2]
    assert [t.tolist() for t in G.row_maps(4)] == [[0, 1, 2, 3]] * 2
    assert G.row_maps(4, 2, 0)[1].tolist() == [1, 2, 4, 5]            # without res_row_mod the residual follows the output row
    a = torch.tensor([[1.0], [2.0], [3.0], [4.0], [5.0], [6.0]], dtype=F64)
    w = torch.tensor([[1.0], [10.0]], dtype=F64)
    res = torch.tensor([[100.0, 200.0], [300.0, 400.0], [500.0, 600.0]], dtype=F64)
    r = G.linear_ref64(a, w, res=res, out_row_group=3, res_row_mod=3)
    assert r["C"].tolist() == [[101, 210], [302, 420], [503, 630], [104, 240], [305, 450], [506, 660]]
    assert r["orow"].tolist() == [1, 2, 3, 5, 6, 7]


def test_wgrad_ref64():
    g = torch.Generator().manual_seed(9)
    dy, x = torch.randn(50, 8, generator=g, dtype=F64), torch.randn(50, 16, generator=g, dtype=F64)
    r = G.wgrad_ref64(dy, x)
    assert (r["C"] - torch.einsum("mn,mk->nk", dy, x)).abs().max().item() <= 1e-12
    assert (r["dbias"] - dy.sum(0)).abs().max().item() <= 1e-12


def test_trunc16_truncates():
    x = 1.0 + 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -9                     # 1.75 bf16 steps above 1: rounds to two steps, truncates to one
    v = torch.tensor([x, -x, 1.5, -3.0, 1.0 + 2.0 ** -11 + 2.0 ** -12])
    assert v.to(BF16).tolist()[:2] == [1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -6)]
    assert G.trunc16(v, BF16).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7), 1.5, -3.0, 1.0]
    assert G.trunc16(v, F16).tolist()[4] == 1.0 and v.to(F16).tolist()[4] == 1.0 + 2.0 ** -10


# ---------------------------------------------------------------------------------------------- routes and coverage
@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "gemm_route_dump.cpp")])
    pairs = G.flat(G.ALL_CASES)
    out = subprocess.run([exe], input="".join(G.dump_line(c, dt) + "\n" for c, dt in pairs), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(pairs)
    return [(c, dt, ln) for (c, dt), ln in zip(pairs, lines)]


def test_every_case_takes_the_kernel_it_is_named_for(plans):
    wrong = [(G.case_id(c, dt), G.plan_text(c), ln) for c, dt, ln in plans
             if (ln.split()[:3] != G.plan_text(c).split() if c["kind"] == "splitk" else ln != G.plan_text(c))]
    assert not wrong, wrong


def test_the_lists_cover_every_routed_kernel(plans):
    tile, g8, g8p, two_tiles, tail = set(), False, set(), False, False
    sk, tn = [], []
    for c, dt, ln in plans:
        f = ln.split()
        if c["kind"] == "linear":
            launches = [f[1 + 4 * i: 5 + 4 * i] for i in range(int(f[0]))]
            tail |= len(launches) == 2 and launches[0][0] == "G8P" and launches[1][0] == "TILE" and int(launches[1][2]) > 0
            for fam, cfg, _, rows in launches:
                if fam == "TILE":
                    tile.add(int(cfg))
                g8 |= fam == "G8"
                if fam == "G8P":
                    g8p.add(int(cfg))
                    two_tiles |= (int(rows) // 256) * (c["N"] // 256) >= 512
        elif c["kind"] == "splitk":
            sk.append(tuple(int(v) for v in f[:3]))
        else:
            tn.append((f[0], int(f[1]), int(f[2])))
    assert tile >= set(range(19)), sorted(set(range(19)) - tile)        # 0-9 routed or behind VMC_GEMM_U / _KS, 10-18 the VMC_GEMM_CFG sweep
    assert g8 and g8p == set(range(8)) and two_tiles and tail
    assert any(s == 1 for s, _, _ in sk) and any(s > 1 and last < per for s, per, last in sk)
    assert any(k == "TN128" and s == 1 for k, s, _ in tn) and any(k == "TN128" and s > 1 for k, s, _ in tn)
    assert any(k == "TN256" and s > 1 for k, s, _ in tn)
    t256 = next(c for c in G.TN_CASES if c["plan"][0] == "TN256")
    assert t256["N"] % 256 and t256["K"] % 256                             # ragged in both tile directions


def test_padded_and_mapped_cases_exist():
    cs = G.ALL_CASES
    for k in ("lda", "ldw", "ldc", "ldres", "ldz"):
        assert any(c["kind"] == "linear" and c["pad"][k] for c in cs), k
    assert any(c["kind"] == "linear" and c["res"] and c["pad"]["ldres"] != c["pad"]["ldc"] for c in cs)
    assert any(c["kind"] == "splitk" and all(c["pad"]) for c in cs) and any(c["kind"] == "tn" and all(c["win"]) for c in cs)
    assert any(c["kind"] == "linear" and c["org"] and c["rrm"] for c in cs)
    assert {c["kind"] for c in cs if c["sub"]} == {"linear", "splitk", "tn"} and all(c["dts"] == (F16,) for c in cs if c["sub"])
    assert all(G.macs(c) <= G.MAX_MACS for c in cs)


# ---------------------------------------------------------------------------------------------- per-case conditions, and the measure on itself
def _f32_evaluation(P):
    """What a float32 evaluation with round-to-nearest stores returns for each output."""
    return {n: (o["r32"] if o["dtype"] is F32 else o["r32"].to(o["dtype"])) for n, o in P["outs"].items()}


def test_conditions_and_f32_evaluation_of_every_case():
    """e32 <= E32_MAX, the pinned share of every 16-bit output, and the rule passes a float32 evaluation (one walk: the cases share
    their float64 products)."""
    bad, seen = [], set()
    for c, dt in G.flat(G.ALL_CASES + G.GROUP_CASES):
        key = (c["kind"], c["M"], c["N"], c["K"], dt, c["sub"], c.get("act"), c.get("bias"), c.get("res"), c.get("out"), c.get("alpha"),
               c.get("org"), c.get("rrm"))
        if key in seen:             # differs from a judged case in Z / a leading dimension / the kernel variant only: the same reference
            continue
        seen.add(key)
        P = G.prepare(c, dt)
        ev = _f32_evaluation(P)
        for n, o in P["outs"].items():
            cid = f"{G.case_id(c, dt)}:{n}"
            if not o["e32"] <= G.E32_MAX:
                bad.append((cid, "e32", o["e32"]))
            if o["dtype"] is not F32 and not o["pinned"] >= G.SHARE_MIN[o["dtype"]]:
                bad.append((cid, "pinned share", o["pinned"]))
            if not G.judge(ev[n], o)["ok"]:
                bad.append((cid, "f32 evaluation fails"))
    assert not bad, bad


def _case(name, cases=None):
    return next(c for c in (cases or G.ALL_CASES) if c["name"] == name)


def _mutant_linear(c, dt, kind):
    """{output: value} of a float32 evaluation of the case with one deliberate mistake."""
    P = G.prepare(c, dt)
    a32, w32 = P["a"].to(F32), P["b"].to(F32)
    bias, res = P["bias"], P["res"]
    p, act, alpha = a32 @ w32.t(), c["act"], c["alpha"]
    if kind == "drop-last-k-tile":
        p = a32[:, :-64] @ w32[:, :-64].t()
    elif kind == "partial-sum-in-16-bits":
        t = a32[:, :64] @ w32[:, :64].t()
        p = (p - t) + t.to(dt).to(F32)
    z = p + bias if (bias is not None and kind != "bias-after-act") else p
    orow, rrow = G.row_maps(c["M"], c["org"], c["rrm"])
    if kind == "alpha-inside-act":
        y = G.R.act_ref(alpha * z, act, F32)
    elif kind == "bias-after-act":
        y = alpha * (G.R.act_ref(z, act, F32) + bias)
    else:
        y = alpha * G.R.act_ref(z, act, F32)
    if res is not None:
        y = y + res.to(F32)[orow.clamp(max=res.shape[0] - 1) if kind == "res-row-by-orow" else rrow]
    zs = G.R.act_ref(z, act, F32) if kind == "z-after-act" else z
    store = (lambda v, t: G.trunc16(v, t)) if kind == "truncating-store" else (lambda v, t: v.to(t))
    odt = P["outs"]["C"]["dtype"]
    return {"C": y if odt is F32 else store(y, odt), "Z": store(zs, dt)}


# mutant -> the cases (by name and dtype) that must reject it
MUTANTS = {
    "truncating-store": [("epi-none-res0-out16-ldc+4", BF16), ("epi-none-res0-out16-ldc+4", F16), ("epi-qgelu-resf32-out16-z-ldc+8", BF16)],
    "alpha-inside-act": [("epi-qgelu-res0-outf32-ldc+4", BF16), ("epi-gelu-res16-out16-ldc+4", F16)],
    "bias-after-act": [("epi-qgelu-res0-outf32-ldc+4", BF16), ("epi-relu-res0-out16-ldc+4", F16)],
    "drop-last-k-tile": [("cfg2-n4", BF16), ("epi-none-res0-outf32-ldc+4", F16)],
    "partial-sum-in-16-bits": [("epi-none-res0-outf32-ldc+4", BF16), ("epi-none-res0-outf32-ldc+4", F16), ("cfg3", BF16)],
    "z-after-act": [("epi-qgelu-res0-out16-z-ldc+4", BF16), ("epi-relu-res0-out16-z-ldc+4", F16)],
    "res-row-by-orow": [("rows-3x16", BF16), ("resmod-245", F16)],
}


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_the_rule_rejects_the_mutant(kind):
    for name, dt in MUTANTS[kind]:
        c = _case(name)
        P = G.prepare(c, dt)
        got = _mutant_linear(c, dt, kind)
        out = "Z" if kind == "z-after-act" else "C"
        assert not G.judge(got[out], P["outs"][out])["ok"], (kind, name, dt)
        sane = _mutant_linear(c, dt, "none")            # the same evaluation without the mistake passes
        assert G.judge(sane[out], P["outs"][out])["ok"], (kind, name, dt)
    if kind == "truncating-store":                      # the issue's figure: a truncating store fails a large share of all elements
        c = _case("epi-none-res0-out16-ldc+4")
        for dt in (BF16, F16):
            m = G.judge(_mutant_linear(c, dt, kind)["C"], G.prepare(c, dt)["outs"]["C"])
            assert m["share_bad"] > 0.25, m


def test_the_rule_rejects_a_dbias_without_the_last_partial_block():
    for name, dt in (("77", BF16), ("4099", F16)):
        c = _case(name, G.TN_CASES)
        P = G.prepare(c, dt)
        whole = (c["M"] // 64) * 64
        assert whole < c["M"]
        o = P["outs"]["dbias"]
        assert not G.judge(P["a"][:whole].to(F32).sum(0), o)["ok"]
        assert G.judge(P["a"].to(F32).sum(0), o)["ok"]
