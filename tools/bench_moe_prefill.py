#!/usr/bin/env python3
"""A/B: HIP prefill of a MoE stage (both MoE MLP paths) vs the torch stage
prefill, on Mixtral-8x7B shapes cut to 4 layers (random bf16 weights).

Per prompt length: one warm-up, then 5 timed runs of each side, the sides
alternating; the median and the spread (max - min) are reported.  Sides:
  torch    stage.forward_head (explicit attention, one torch.where per
           expert per layer)
  hip/0    DecodeEngine.prefill_prompt, moe_prefill_group_max = 0
           (expert-major library GEMMs)
  hip/128  the same with moe_prefill_group_max = 128 (grouped decode
           kernels), for T <= 128
The crossover is the largest candidate in {0, 16, 32, 64, 128} below which
the grouped path's median is the lower one at every measured length.  The
gate: with that crossover the HIP median is at most the torch median plus
the torch spread at every length.  Prints a table and one JSON line;
--out also writes the JSON to a file."""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

LENGTHS = (16, 32, 64, 128, 512, 2048, 4096)
CANDIDATES = (0, 16, 32, 64, 128)
RUNS = 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--lengths", type=int, nargs="*", default=list(LENGTHS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from mdi_llm_amd.config import ModelConfig
    from mdi_llm_amd.models.stages import StarterStage
    from mdi_llm_amd.ops.engine import DecodeEngine

    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    cfg = ModelConfig.from_name("Mixtral-8x7B-v0.1", n_layer=args.layers)
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        stage = StarterStage(cfg, cfg.n_layer)
    torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for p in stage.parameters():
            p.normal_(0, 0.02)
    stage.max_seq_length = max(args.lengths)
    stage.eval()
    stage.set_kv_cache(1)
    eng = DecodeEngine(stage, stage.kv_pool, use_graphs=False)
    assert eng.supports_hip_prefill

    rows = []
    for T in args.lengths:
        toks = torch.randint(0, cfg.vocab_size, (T,), device=dev)

        def ref():
            with torch.inference_mode():
                stage.forward_head(toks.view(1, -1), slot=0, input_pos=0)

        def hip(group_max):
            def run():
                eng.moe_prefill_group_max = group_max
                eng.prefill_prompt(toks, 0, 0)
            return run

        sides = {"torch": ref, "hip/0": hip(0)}
        if T <= 128:
            sides["hip/128"] = hip(128)
        for fn in sides.values():  # warm-up: code objects, GEMM algorithms
            timed(fn)
        ms = {name: [] for name in sides}
        for _ in range(RUNS):       # alternate the sides
            for name, fn in sides.items():
                ms[name].append(timed(fn))
        row = {"T": T}
        for name, v in ms.items():
            row[name] = {"median_ms": statistics.median(v),
                         "spread_ms": max(v) - min(v)}
        rows.append(row)
        print(f"T={T:5d} " + "  ".join(
            f"{name}: {r['median_ms']:9.3f} ms (+-{r['spread_ms']:.3f})"
            for name, r in row.items() if name != "T"), flush=True)

    # crossover: the grouped path must win at every measured T <= candidate
    short = [r for r in rows if "hip/128" in r]
    crossover = 0
    for c in CANDIDATES[1:]:
        at = [r for r in short if r["T"] <= c]
        if not at or not all(
                r["hip/128"]["median_ms"] < r["hip/0"]["median_ms"]
                for r in at):
            break
        crossover = c
    gate = []
    for r in rows:
        side = "hip/128" if r["T"] <= crossover else "hip/0"
        ok = r[side]["median_ms"] <= (r["torch"]["median_ms"]
                                      + r["torch"]["spread_ms"])
        gate.append({"T": r["T"], "side": side, "pass": ok})
        if not ok:
            print(f"GATE MISSED at T={r['T']}: {side} "
                  f"{r[side]['median_ms']:.3f} ms vs torch "
                  f"{r['torch']['median_ms']:.3f} ms")
    result = {"model": cfg.name, "n_layer": cfg.n_layer,
              "device": torch.cuda.get_device_name(0), "runs": RUNS,
              "rows": rows, "crossover": crossover, "gate": gate}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
