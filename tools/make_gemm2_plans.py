"""tools/tune_gemm2.py output (JSON lines) -> comat_amd/csrc/gemm2_plans.inc (the static plan table of gemm2.hip).
    python tools/make_gemm2_plans.py [--base old_plans.inc] gpurun_out/g2_tune.jsonl [more.jsonl ...]
Per problem the fastest measured (tile, splits); among variants within 3 % of the fastest the one with the fewest slices
(less slab traffic, least sensitivity to what else runs on the chip).  Tile codes above 13 never enter gemm2_plans.inc:
    python tools/make_gemm2_plans.py --wide [--table report.txt] g2_tune_wide.jsonl [more.jsonl ...]
writes comat_amd/csrc/gemm2_plans_wide.inc from the output of TUNE_WIDE=1 tools/tune_gemm2.py: a row per problem whose wide shape
(code 14) beat the plan of gemm2_plans.inc in the alternating measurement by more than the spread (max - min) of either
list of times - and whose slices cut k where the slices of that plan cut it: every output element is then the same sum of the same
partial sums in the same order (all shapes run the same MFMA k-steps in k order), so a row changes the time of a launch and not one
bit of its result.  --table also writes every measured problem with both lists."""
import json
import re
import sys

rows = {}
args = sys.argv[1:]
if args and args[0] == "--wide":
    args = args[1:]
    table = None
    if args and args[0] == "--table":
        table, args = args[1], args[2:]
    mean = lambda v: sum(v) / len(v)
    cdiv = lambda a, b: -(-a // b)

    def k_cuts(plan, nkt):
        """the k positions (in 64-byte k-tiles) at which plan "code:slices" cuts a contraction of nkt k-tiles (plan2 + finish_launch
        + the kernel's own division: codes 8 - 11 and 14 count 128-byte tiles, 12 and 13 are never split)"""
        code, sl = (int(v) for v in plan.split(":"))
        if code == 0:
            return None  # no row in gemm2_plans.inc: the rule of thumb's plan is not reproduced here
        unit = 2 if code in (8, 9, 10, 11, 14) else 1
        n = nkt // unit
        sl = 1 if code in (12, 13) else max(1, min(sl, n, 32))
        per = cdiv(n, cdiv(n, cdiv(n, sl)))
        return [min(i * per, n) * unit for i in range(cdiv(n, per) + 1)]
    seen = {}
    for path in args:
        for line in open(path):
            if line.startswith("{") and '"wide_us"' in line:
                r = json.loads(line)
                key = ({"conv": 1, "gemm8": 2, "conv8": 3}.get(r["kind"], 0), r["M"], r["N"], r["nkt"], r["batch"])
                if key not in seen or r["calls"] >= seen[key]["calls"]:
                    seen[key] = r
    report = ["# kind M N k-tiles batch | calls | plan of gemm2_plans.inc: us per launch (alternating) | wide shape: us per launch | "
              "mean gain us, spread us, verdict"]
    for key, r in sorted(seen.items(), key=lambda kv: -kv[1]["calls"] * (mean(kv[1]["base_us"]) - mean(kv[1]["wide_us"]))):
        b, w = r["base_us"], r["wide_us"]
        gain, spread = mean(b) - mean(w), max(max(b) - min(b), max(w) - min(w))
        same = k_cuts(r["base"], r["nkt"]) is not None and k_cuts(r["base"], r["nkt"]) == k_cuts(r["wide"], r["nkt"])
        win = gain > spread and same
        report.append(f"{key[0]} {key[1]:6d} {key[2]:6d} {key[3]:4d} {key[4]:2d} | {r['calls']:4d} | {r['base']:>5s}: {' '.join(f'{v:.2f}' for v in b)} | "
                      f"{r['wide']:>5s}: {' '.join(f'{v:.2f}' for v in w)} | {gain:+.2f} {spread:.2f} {'row' if win else '-' if same else '- (other k cuts)'}")
        if win:
            c, s = (int(v) for v in r["wide"].split(":"))
            rows[key] = (c, s, mean(w), mean(b), r["calls"], r["calls"] * gain)
    out = ["// gemm2_plans_wide.inc - measured plans that choose tile code 14 (128x128, 8 waves, 128-byte k-tiles):",
           "// TUNE_WIDE=1 tools/tune_gemm2.py on an MI355X -> tools/make_gemm2_plans.py --wide.  Same row format as gemm2_plans.inc; plan2",
           "// searches this table first.  A row stands here only where the new shape beat the problem's plan of gemm2_plans.inc by more than",
           "// the spread of the alternating measurement AND cuts k into the same slices as that plan: the results of a launch are then the",
           "// parent plan's bit for bit.  Trailing comment: us per launch with this plan, with the plan of gemm2_plans.inc, calls per step.",
           "static const Plan2Entry g2_plans_wide[] = {"]
    for key in sorted(rows, key=lambda k: -rows[k][5]):
        c, s, us, base, calls, _ = rows[key]
        out.append(f"    {{{key[0]}, {key[1]}, {key[2]}, {key[3]}, {key[4]}, {c}, {s}}},  // {us:.1f} us (gemm2_plans.inc {base:.1f}), {calls} calls")
    out.append("};")
    if table:
        open(table, "w").write("\n".join(report) + "\n")
    print(f"{len(seen)} problems measured, {len(rows)} rows; modelled step gain {sum(v[5] for v in rows.values()) / 1e3:.2f} ms")
    if rows:  # (an empty table is no table: the two shapes then have no user and leave the kernel)
        open("comat_amd/csrc/gemm2_plans_wide.inc", "w").write("\n".join(out) + "\n")
    sys.exit(0)
if args and args[0] == "--base":  # keep the entries of an existing table (problems the given measurements do not cover)
    for m in re.finditer(r"^\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},\s*// ([\d.]+) us \(general ([\d.]+)\), (\d+) calls",
                         open(args[1]).read(), re.M):
        v = m.groups()
        rows[tuple(int(x) for x in v[:5])] = (int(v[5]), int(v[6]), float(v[7]), int(v[9]), float(v[8]), args[1])
    args = args[2:]
for path in args:
    for line in open(path):
        if not line.startswith("{"):
            continue
        r = json.loads(line)
        if "wide_us" in r:
            continue
        key = ({"conv": 1, "gemm8": 2, "conv8": 3}.get(r["kind"], 0), r["M"], r["N"], r["nkt"], r["batch"])
        var = {k: v for k, v in r["us"].items() if ":" in k and int(k.split(":")[0]) <= 13}  # (codes above 13: --wide)
        best = min(var.values())
        ok = [(int(k.split(":")[1]), v, k) for k, v in var.items() if v <= best * 1.03]
        s, us, k = min(ok)
        cfg = int(k.split(":")[0])
        old = rows.get(key)
        if old is None or r["calls"] >= old[3] or path != old[5]:  # later files (newer measurements) win
            rows[key] = (cfg, s, us, max(r["calls"], old[3] if old else 0), r["us"].get("general", 0.0), path)
out = ["// gemm2_plans.inc - measured plans of the pipelined GEMM / conv kernel for the problems of the SD1.5 (C2) and SDXL (C4) steps:",
       "// tools/tune_gemm2.py on an MI355X -> tools/make_gemm2_plans.py.  {kind, M, N, k-tiles, batch, tile code, slices}; kind 0 GEMM, 1 conv,",
       "// 2 / 3 the same with fp8 operands (C5; k-tiles of 64 bytes either way)",
       "// tile codes: 1 128x128, 2 128x64, 3 256x128, 4 64x128, 6 64x64, 7 128x128 with 8 waves; 8..11 = 64x64, 128x64, 64x128, 128x128 with",
       "// 128-byte k-tiles; 12 256x256, 13 256x128 (wave tiles of 128x64, never split).  Trailing comment: us per launch with this plan,",
       "// with the general 64x64 kernel, calls per step.",
       "static const Plan2Entry g2_plans[] = {"]
for key in sorted(rows, key=lambda k: (-rows[k][3] * rows[k][2])):
    cfg, s, us, calls, gen, _ = rows[key]
    out.append(f"    {{{key[0]}, {key[1]}, {key[2]}, {key[3]}, {key[4]}, {cfg}, {s}}},  // {us:.1f} us (general {gen:.1f}), {calls} calls")
out.append("};")
open("comat_amd/csrc/gemm2_plans.inc", "w").write("\n".join(out) + "\n")
print(f"{len(rows)} plans; step total {sum(v[2] * v[3] for v in rows.values()) / 1e3:.1f} ms "
      f"(general kernel {sum(v[4] * v[3] for v in rows.values()) / 1e3:.1f} ms)")
