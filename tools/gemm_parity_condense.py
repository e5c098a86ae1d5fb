"""Reduce the per-case figures of tests/test_gpu_gemm_parity.py (VMC_GEMM_PARITY_JSON=<file>) to the tables of profiles/gemm_parity.md:
the worst ratio per kernel family, dtype and output type, and the share of bit-pinned elements per 16-bit family.

    python tools/gemm_parity_condense.py profiles/gemm_parity.jsonl"""
import collections
import json
import sys


def main(path):
    rows = [json.loads(ln) for ln in open(path)]
    worst = collections.OrderedDict()
    for r in rows:
        if "ratio" not in r:
            continue
        k = (r["family"], r["dtype"], r["out_dtype"])
        w = worst.setdefault(k, dict(n=0, ratio=-1.0, case="", pin_lo=1.0, pin_hi=0.0, outside=0))
        w["n"] += 1
        if r["ratio"] > w["ratio"]:
            w["ratio"], w["case"] = r["ratio"], f"{r['case']}:{r['output']}"
        if "pinned" in r:
            w["pin_lo"], w["pin_hi"] = min(w["pin_lo"], r["pinned"]), max(w["pin_hi"], r["pinned"])
            w["outside"] += r["bad"]
    print("| family | operands | output | checked outputs | worst ratio (8 allowed) | bit-pinned share | elements outside |")
    print("|---|---|---|---|---|---|---|")
    for (fam, dt, odt), w in sorted(worst.items(), key=lambda kv: (kv[0][0].rstrip("0123456789"), len(kv[0][0]), kv[0])):
        pin = "-" if odt == "f32" else f"{w['pin_lo']:.3f} - {w['pin_hi']:.3f}"
        print(f"| {fam} | {dt} | {odt} | {w['n']} | {w['ratio']:.2f} ({w['case']}) | {pin} | {'-' if odt == 'f32' else w['outside']} |")
    kept = sum(1 for r in rows if r["sentinel_kept"])
    print(f"\n{len(rows)} lines, {kept} with the sentinel intact.")


if __name__ == "__main__":
    main(sys.argv[1])
