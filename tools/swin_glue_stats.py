#!/usr/bin/env python3
"""Turn rocprofv3's per-kernel statistics of one `tools/swin_time.py --autocast --glue --only autocast_bf16_glue` run (Swin-L
384_22k, 32 frames of 224^2, bf16 autocast, MSDA_SWIN_BF16=1 and MSDA_SWIN_GLUE=1) into profiles/swin_glue_kernel_stats.csv:
one row per glue kernel with the bytes it must move per step, computed from the model's shapes below, and the share of the
measured HBM rate that gives; then the Swin attention kernels and every other kernel of the step summed by kind.

    rocprofv3 --kernel-trace --stats -d DIR -o glue --output-format csv -- python tools/swin_time.py --autocast --glue \\
        --only autocast_bf16_glue --steps 2 --warmup 1 --no-counts --out ""
    python tools/swin_glue_stats.py DIR/glue_kernel_stats.csv --steps 3 > profiles/swin_glue_kernel_stats.csv

(--glue-stages 4 for a profile of the fp32 route `--glue --only dropin_glue`.)  A profile of `--glue-stream --only
autocast_bf16_glue_stream` (MSDA_SWIN_GLUE_BF16=1 as well) needs no option: the kernels of a bf16 residual stream are other
instantiations (X = unsigned short), counted with 2-byte rows over stages 1 to 3.

Bytes a kernel must move per row element (x, y and their gradients: X = fp32 = 4 or bf16 = 2; T = bf16 = 2; statistics and
parameters left out), for X = fp32: norm forward x + z = 6, backward grad_z + x + grad_x = 10; add + norm forward x + a + y + z =
12, backward grad_y + grad_z + y + grad_x + grad_a = 16; add forward x + a + y = 10, backward grad_y + grad_a = 6; merge + norm
forward (per element of the 4C-wide row) x + z = 6, backward 10; with T = fp32 each T term is 4 instead of 2, with X = bf16 each
X term is 2 instead of 4, and add + norm's backward without a keep vector writes no grad_a (it is grad_x; counted as written, so
the share of the HBM rate is an upper bound there).  A kernel's bytes per step are its calls per step
times the bytes of its stage's rows, so checkpoint recomputation and the per-stage output norms are counted as they ran."""
import argparse
import csv
import re
import sys

FRAMES = 32
STAGES = ((56, 56, 192, 2), (28, 28, 384, 2), (14, 14, 768, 18), (7, 7, 1536, 2))      # H, W, C, depth at 224^2
HBM_TBS = 6.29                                                                          # measured float4 copy rate, TB/s
NV_WIDTH = {1: 256, 2: 512, 3: 768, 4: 1024, 6: 1536, 8: 2048, 12: 3072}


def stage_of_width(width, merged):
    """(rows, blocks) of the stage whose rows (or merged rows) have this width."""
    for H, W, C, depth in STAGES:
        if not merged and C == width:
            return FRAMES * H * W, depth
        if merged and 4 * C == width:
            return FRAMES * ((H + 1) // 2) * ((W + 1) // 2), depth
    return None, None


def width_of(nv, merged):
    lo = max([0] + [w for n, w in NV_WIDTH.items() if n < nv])
    for H, W, C, _ in STAGES:
        width = 4 * C if merged else C
        if lo < width <= NV_WIDTH[nv]:
            return width
    return None


def must_move(name, calls_per_step, glue_stages):
    """(label, bytes per step) of a glue kernel from its template arguments and its calls per step, or None.  A kernel whose
    width is a template argument serves one stage, so its calls all move the same bytes; the add kernels serve every stage
    that takes the glue (`glue_stages`: 4 in fp32, 1 under autocast, where the stream is fp32 in stage 0 only)."""
    m = re.search(r"glue_(fwd|bwd)_kernel<(\d+), *(unsigned short|float), *(unsigned short|float), *(\d)>", name)
    if m:
        direction, nv, stream, typ, mode = m.group(1), int(m.group(2)), m.group(3), m.group(4), int(m.group(5))
        t = 2 if typ == "unsigned short" else 4
        xb = 2 if stream == "unsigned short" else 4
        merged = mode == 2
        width = width_of(nv, merged)
        rows, _ = stage_of_width(width, merged)
        if rows is None:
            return None
        op = ("norm", "add_norm", "merge_norm")[mode]
        per_elem = {("norm", "fwd"): xb + t, ("norm", "bwd"): t + 2 * xb, ("add_norm", "fwd"): 2 * xb + 2 * t,
                    ("add_norm", "bwd"): 3 * xb + 2 * t, ("merge_norm", "fwd"): xb + t,
                    ("merge_norm", "bwd"): t + 2 * xb}[(op, direction)]
        label = "glue %s %s width %d %s%s" % (op, "forward" if direction == "fwd" else "backward", width,
                                              "bf16" if t == 2 else "fp32", " (bf16 stream)" if xb == 2 else "")
        return label, calls_per_step * rows * width * per_elem
    m = re.search(r"glue_add_(fwd|bwd)_kernel<(unsigned short|float), *(unsigned short|float)>", name)
    if m:
        # The first block of the network has no drop-path: its closing add saves nothing, so checkpoint recomputation stops
        # before it (forward: once instead of twice), and in fp32 its grad_a is grad_y itself (no launch).
        direction, t = m.group(1), 2 if m.group(3) == "unsigned short" else 4
        xb = 2 if m.group(2) == "unsigned short" else 4
        per_elem = 2 * xb + t if direction == "fwd" else xb + t
        calls, total = 0, 0
        # a bf16 stream: stages 1 to 3 (every block there has drop-path), whatever glue_stages says of the fp32 stream
        first, stages = (1, STAGES[1:]) if xb == 2 else (0, STAGES[:glue_stages])
        for i, (H, W, C, depth) in enumerate(stages, first):
            n = 2 * depth - (i == 0) if direction == "fwd" else depth - (i == 0 and t == 4)
            calls += n
            total += n * FRAMES * H * W * C * per_elem
        label = "glue add %s (%d stage%s) %s%s" % ("forward" if direction == "fwd" else "backward", len(stages),
                                                   "" if len(stages) == 1 else "s", "bf16" if t == 2 else "fp32",
                                                   " (bf16 stream)" if xb == 2 else "")
        if abs(calls - calls_per_step) > 1e-9:
            label += " (%g calls per step, %d expected: bytes not comparable)" % (calls_per_step, calls)
        return label, total
    return None


def kind_of(name):
    if "glue_param_reduce" in name:
        return "glue parameter-gradient reduce"
    if re.search(r"swin_(fwd|bwd)", name):
        return None
    if re.search(r"Cijk_|gemm|Gemm|GEMM", name):
        return "vendor GEMMs (hipBLASLt)"
    if re.search(r"layer_norm|LayerNorm|RowwiseMoments|GammaBeta", name):
        return "LayerNorm forward / backward (torch, fp32)"
    if "copy_kernel" in name:
        return "fp32 <-> bf16 casts and copies (torch)"
    return "other element-wise and reductions (torch)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stats", help="rocprofv3's <name>_kernel_stats.csv")
    ap.add_argument("--steps", type=int, default=3, help="backbone steps in the profiled run (warm-up included)")
    ap.add_argument("--glue-stages", type=int, default=1,
                    help="stages whose residual stream is fp32 and takes the glue: 1 under bf16 autocast (default), 4 in fp32")
    args = ap.parse_args()
    rows = list(csv.DictReader(open(args.stats)))
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "calls", "avg_us", "min_us", "max_us", "ms_per_step", "must_move_mb_per_step", "achieved_tb_per_s",
                  "share_of_hbm_rate"])
    kinds, total_calls, total_ms = {}, 0, 0.0
    named = []
    for r in rows:
        name, calls, total_ns = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        ms = total_ns / 1e6 / args.steps
        total_calls += calls
        total_ms += ms
        moved = must_move(name, calls / args.steps, args.glue_stages)
        if moved:
            label, nbytes = moved
            tbs = nbytes / (ms * 1e-3) / 1e12
            named.append((ms, [label, calls, round(total_ns / calls / 1e3, 1), round(float(r["MinNs"]) / 1e3, 1),
                               round(float(r["MaxNs"]) / 1e3, 1), round(ms, 3), round(nbytes / 1e6, 1), round(tbs, 2),
                               round(tbs / HBM_TBS, 2)]))
            continue
        kind = kind_of(name)
        if kind is None:
            short = re.search(r"swin_\w+", name).group(0)
            named.append((ms, [short, calls, round(total_ns / calls / 1e3, 1), round(float(r["MinNs"]) / 1e3, 1),
                               round(float(r["MaxNs"]) / 1e3, 1), round(ms, 3), "", "", ""]))
            continue
        k = kinds.setdefault(kind, [0, 0.0])
        k[0] += calls
        k[1] += ms
    for _, row in sorted(named, key=lambda t: -t[0]):
        out.writerow(row)
    for kind, (calls, ms) in sorted(kinds.items(), key=lambda kv: -kv[1][1]):
        out.writerow([kind, calls, round(ms * args.steps * 1e3 / calls, 1), "", "", round(ms, 3), "", "", ""])
    out.writerow(["all kernels", total_calls, "", "", "", round(total_ms, 3), "", "", ""])


if __name__ == "__main__":
    main()
