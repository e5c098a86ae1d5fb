"""Condense the per-case file tests/test_gpu_attention_parity.py writes (VMC_ATTN_PARITY_JSON=<path>) into the lines of
profiles/attention_parity.jsonl: per test list (family), dtype and output the worst rms and max ratio against the model with the
case that gave it (scalar kernels: the worst share of their e32 bound), after the margins line.  With --markdown the same as the
table of profiles/attention_parity.md.  The mutation lines of the committed file cannot be regenerated (the mutated trees are not
kept): pass the old file as the third argument to carry them over.

    python tools/attn_parity_condense.py per_case.jsonl > condensed.jsonl
"""
import collections
import json
import sys


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = [json.loads(l) for l in open(args[0])]
    head, rows = rows[0], rows[1:]
    agg = collections.OrderedDict()
    for r in rows:
        fam = r["family"]
        if fam.startswith("attn_vit_kernel/variant"):
            fam = "attn_vit_kernel (VMC_ATTN_VARIANT 2..23)"
        a = agg.setdefault((fam, r["dtype"], r["output"]), dict(n=0, rms=0.0, max=0.0, excess=0.0, case_rms="", case_max=""))
        a["n"] += 1
        where = r["case"] + "/" + r["way"]
        if "excess" in r:
            if r["excess"] >= a["excess"]:
                a["excess"], a["case_max"] = r["excess"], where
        else:
            if r["ratio_rms"] >= a["rms"]:
                a["rms"], a["case_rms"] = r["ratio_rms"], where
            if r["ratio_max"] >= a["max"]:
                a["max"], a["case_max"] = r["ratio_max"], where
    md = "--markdown" in sys.argv
    if md:
        print("| family | dtype | output | cases | worst rms ratio | worst max ratio |\n|---|---|---|---|---|---|")
    else:
        print(json.dumps(dict(kind="margins", R_RMS=head["R_RMS"], R_MAX=head["R_MAX"], vacuity_max=0.25, vacuity_rms=0.1,
                              note="fixed before the first GPU run; not calibrated on a kernel")))
    for (fam, dt, o), a in agg.items():
        if fam.endswith("/scalar"):
            if md:
                print(f"| {fam} | {dt} | {o} | {a['n']} | - | {a['excess']:.2f} of the e32 bound ({a['case_max']}) |")
            else:
                print(json.dumps(dict(kind="scalar", family=fam, dtype=dt, output=o, cases=a["n"], worst_excess=round(a["excess"], 4),
                                      case=a["case_max"])))
        elif md:
            print(f"| {fam} | {dt} | {o} | {a['n']} | {a['rms']:.2f} ({a['case_rms']}) | {a['max']:.2f} ({a['case_max']}) |")
        else:
            print(json.dumps(dict(kind="measure", family=fam, dtype=dt, output=o, cases=a["n"], worst_ratio_rms=round(a["rms"], 4),
                                  case_rms=a["case_rms"], worst_ratio_max=round(a["max"], 4), case_max=a["case_max"])))
    if len(args) > 1 and not md:
        for l in open(args[1]):
            if json.loads(l).get("kind") == "mutation":
                print(l, end="")


if __name__ == "__main__":
    main()
