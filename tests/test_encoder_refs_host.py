"""CPU checks of tests/encoder_refs.py: the float64 forward against oracle/vit.py in float64 on every stage and its attention against
attention_refs' closed form, the kernels every case reaches (gemm_route.h through tests/host/gemm_route_dump.cpp, attn_route.h
through attention_refs' port), the conditions that make the measure mean something (for every case and dtype), the measure on a
float32 evaluation of the model, and twelve mutants of that evaluation that it must catch."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_refs as AR                      # noqa: E402
import encoder_refs as R                         # noqa: E402
from oracle import vit as ovit                   # noqa: E402
from train_kernel_refs import BF16, DT_NAME, F16      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
DTYPES = (BF16, F16)
CONFIGS = [(c["name"], dt) for c in R.CASES for dt in DTYPES]
CFG_ID = lambda v: v if isinstance(v, str) else DT_NAME[v]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _refs(name, dtype):
    """(reference restricted to the tensors the case compares, model)."""
    r, m = R.forward_ref64(name, dtype), R.forward_model16(name, dtype)
    assert list(m) == R.output_names(R.BY_NAME[name])
    return dict({n: r[n] for n in m}, floor=r["floor"]), m


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_ref64_is_the_oracle_in_float64_on_every_stage(name):
    """ln_pre, both residual adds of every block and the embeddings to 1e-12 relative, on the 16-bit weight copies widened, the fp32
    master conv1 and the pixels through the wrap quirk where the case has it."""
    inp, r = R.make_inputs(name, BF16), R.forward_ref64(name, BF16)
    c = inp["case"]
    sd = {n: (inp["w16"][n] if n in inp["w16"] else inp["p32"][n]).to(F64) for n in R.param_shapes(c)}
    fr = R.frames_rgb(inp)
    trace = []
    emb = ovit.vit_forward(sd, ovit.normalize_u8(ovit.to_pil_wrap_u8(fr) if c["wrap"] else fr, F64), c["H"], trace=trace, dtype=F64)
    assert [n for n, _ in trace] == ["ln_pre"] + [f"blk{i}.{s}" for i in range(c["L"]) for s in ("attn", "mlp")]
    for n, t in trace:
        assert _rel(r[n], t.reshape(r[n].shape)) <= 1e-12, n
    assert _rel(r["E"], emb) <= 1e-12
    assert set(R.stage_names(c)) <= {n for n, _ in trace}


@pytest.mark.parametrize("F,N,NQ", [(3, 17, 17), (2, 65, 65), (3, 50, 1)])
def test_attention_piece_is_attention_refs_closed_form(F, N, NQ):
    """The attention the reference calls (all queries, and the class query on K | V) equals attn_ref64's out on a packed qkv."""
    H, D = 4, 256
    qkv = AR.vit_random(F, N, H, BF16, 5).to(F64)
    q, k, v = AR.vit_split(qkv, H)
    if NQ == 1:
        q = q.reshape(F, N, D)[:, 0].contiguous()
    out = R.vit_forward(q, k, v, (F, H, NQ, N, 64))["out"]
    ref = AR.attn_ref64(q, k, v, None, torch.zeros_like(q), shape=(F, H, NQ, N, 64))
    assert _rel(out, ref["out"]) <= 1e-12


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "host", "gemm_route_dump.cpp")])
    calls = [(c["name"], dt, what, line) for c in R.CASES for dt in DTYPES for what, line in R.gemm_calls(c, dt)]
    out = subprocess.run([exe], input="".join(line + "\n" for *_, line in calls), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(calls)
    return {(n, dt, what): ln for (n, dt, what, _), ln in zip(calls, lines)}


def test_cases_reach_the_gemm_kernels_they_are_listed_for(plans):
    """gemm_route.h itself: case l has the bench's routes (the persistent walk on 195 tiles, the walk plus its small-tile tail launch
    on 260, the one-tile-per-workgroup 8-phase kernel on 130); every other call of every case is one small-tile launch."""
    assert not [k for k, ln in plans.items() if ln.startswith("rc")]
    for dt in DTYPES:
        assert plans[("l", dt, "blk0.in_proj")] == "1 G8P 0 0 16640"
        f = plans[("l", dt, "blk0.c_fc")].split()
        assert f[:5] == ["2", "G8P", "2", "0", "16384"] and f[5] == "TILE" and f[7:] == ["16384", "256"], f
        assert plans[("l", dt, "blk1.kv")] == "1 G8 0 0 16640"
    big = {k for k, ln in plans.items() if not ln.startswith("1 TILE")}
    assert big == {("l", dt, w) for dt in DTYPES for w in ("blk0.in_proj", "blk0.c_fc", "blk1.kv")}, big
    # the strided class rows: lda = N D for the q third, ldc = ldres = N D for the unfused epilogues (cases g, r1, r2)
    for name in ("g", "r1", "r2"):
        c = R.BY_NAME[name]
        f = dict(R.gemm_calls(c, BF16))["blk1.c_proj"].split()
        assert not c["fused"] and int(f[6]) == int(f[7]) == c["N"] * c["D"] and f[11] == "1"
    f = dict(R.gemm_calls(R.BY_NAME["a"], BF16))["blk1.q_cls"].split()
    assert int(f[4]) == 17 * 256


def test_cases_reach_the_attention_kernels_and_paths_they_are_listed_for():
    want = {"a": (17, 7), "b": (50, 6), "c": (65, 9), "d": (197, 5), "e": (257, 0), "g": (17, 7), "h": (50, 6), "i": (17, 7), "j": (17, 7),
            "k": (65, 9), "l": (65, 9), "m": (17, 7), "r1": (17, 7), "r2": (65, 9)}
    for name, (N, inst) in want.items():
        c = R.BY_NAME[name]
        assert c["N"] == N and R.route_vit(N, N, c["F"], c["H"])[:2] == ("ATTN_VIT", inst), name
        assert R.route_vit(N, 1, c["F"], c["H"])[:2] == ("ATTN_VIT", 4 if N == 257 else inst)
    f = R.BY_NAME["f"]
    assert f["N"] == 577 and R.route_vit(577, 577, f["F"], f["H"])[:2] == ("ATTN_VIT_LONG", 577)
    assert R.route_vit(577, 1, f["F"], f["H"])[:2] == ("ATTN_VIT_LONG_CLS", 577)
    by = R.BY_NAME
    assert [n for n, c in by.items() if not c["fused"]] == ["g", "r1", "r2"] and [n for n, c in by.items() if c["res16"]] == ["r1", "r2"]
    assert {n: c["mode"] for n, c in by.items() if c["mode"] != "u8_exact"} == {"d": "f32_split", "k": "plain"}
    assert (by["b"]["kpad"], by["d"]["K"], by["d"]["kpad"]) == (192, 48, 64)
    assert [n for n, c in by.items() if c["wrap"]] == ["c"] and [n for n, c in by.items() if c["defer"]] == ["h"]
    assert [n for n, c in by.items() if not c["cls_query"]] == ["i"] and [n for n, c in by.items() if not c["cls_only"]] == ["h", "i"]
    assert by["j"]["D"] == 3 * 256 and by["m"]["F"] == 5 and by["m"]["frame_chunk"] == 2 and by["l"]["F"] * by["l"]["N"] == 16640
    assert by["h"]["seed"] == by["b"]["seed"] and torch.equal(R.make_inputs("h", BF16)["frames"], R.make_inputs("b", BF16)["frames"])
    assert R.stage_names(by["a"]) == ["ln_pre", "blk0.attn", "blk0.mlp"] and R.stage_names(by["i"])[-1] == "blk1.attn"


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_inputs_make_the_measure_mean_something(name, dtype):
    """From the two references alone: 2 rms(E) <= 0.1 rms(r64) for every tensor; 4 max|E| <= 0.25 rms(r64) for every f16 tensor and
    for at least three quarters of the bf16 tensors; attention not trivially uniform; the wrap case's frames hold every pixel value."""
    inp, full = R.make_inputs(name, dtype), R.forward_ref64(name, dtype)
    r, m = _refs(name, dtype)
    c = inp["case"]
    bad_rms, bad_max = R.vacuity(r, m)
    n = len(m)
    print(f"{name} {DT_NAME[dtype]}: {n} tensors, stress {inp['stress']}, max condition missed by {bad_max}")
    assert not bad_rms, bad_rms
    if dtype == F16:
        assert not bad_max, bad_max
    else:
        assert 4 * len(bad_max) <= n, bad_max
    assert len(full["attn_peak"]) == c["L"] and min(full["attn_peak"]) >= 4.0 / c["N"], full["attn_peak"]
    if c["wrap"]:
        v = inp["frames"].to(torch.int64)
        assert len(torch.unique(v)) == 256 and bool((v == 0).any()) and bool((v > 0).any())      # 0 -> 0 and v -> 256 - v
    for k in m:
        assert torch.isfinite(r[k]).all() and torch.isfinite(m[k]).all() and float(r[k].abs().max()) > 0, k
    if c["mode"] != "plain" and not c["res16"]:
        # the split-precision patch GEMM's designed error after ln_pre is far below a 16-bit rounding: under 2^-16 of the stream, where dropping the
        # lo half of the weights leaves 2^-9 (bf16) or 2^-12 (f16)
        assert float((m["ln_pre"] - r["ln_pre"]).abs().max()) <= 2.0 ** -16 * float(r["ln_pre"].abs().max())


@pytest.mark.parametrize("name,dtype", CONFIGS, ids=CFG_ID)
def test_measure_passes_a_float32_evaluation_of_the_model(name, dtype):
    r, m = _refs(name, dtype)
    ms, bad = R.check(R.forward_eval32(name, dtype), r, m)
    assert len(ms) == len(m)
    print(f"{name} {DT_NAME[dtype]}: float32 self-evaluation, worst rms ratio {max(x['ratio_rms'] for x in ms):.3f}, "
          f"worst max ratio {max(x['ratio_max'] for x in ms):.3f}")
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=CFG_ID)
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_measure_catches_the_mutants(mutant, dtype):
    """Each wrong forward fails the case named for it on the tensor named for it, in both dtypes."""
    name, tensor = R.MUTANT_CASE[mutant]
    r, m = _refs(name, dtype)
    ms, bad = R.check(R.forward_eval32(name, dtype, bug=mutant), r, m)
    hit = next(x for x in ms if x["name"] == tensor)
    print(f"{mutant} on case {name} {DT_NAME[dtype]}: {tensor} rms ratio {hit['ratio_rms']:.3g}, max ratio {hit['ratio_max']:.3g}; "
          f"{len(bad)} tensors fail")
    assert not hit["ok"], f"{mutant} passes case {name} on {tensor} in {DT_NAME[dtype]}"
