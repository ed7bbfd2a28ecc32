#!/usr/bin/env python3
"""A/B: HIP prefill (rope-append + MFMA causal flash attention) vs the
torch stage prefill (matmul+softmax, S^2 scores), random-init bf16.

  bench_prefill.py [--model NAME] [--lengths 512,2048] [--rounds 2] [--reps 3]

Prompt lengths are clamped to the model's block size.  Every shape is warmed
up on both paths first; then the two paths alternate, `rounds` times, each
timing one window of `reps` prefills that ends in a synchronise.  Per length
it prints every window, and torch/hip of the window means with the spread
(max - min) / mean of each path's repeats beside it.

  bench_prefill.py --batch N --lengths 32 ...

times N prompts of each length instead: the per-prompt loop against the
packed pass with and without the varlen kernels (bench_batch)."""

import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def bench_batch(args, cfg, eng, lengths, dev):
    """--batch N: N prompts of T tokens into slots 0..N-1, three ways:
    loop (prefill_prompt per prompt), packed+loop (packed GEMMs, attention
    per sequence: MDI_PREFILL_VARLEN_ATTN=0) and packed+varlen.  The paths
    alternate in one process; the median window of each is reported."""
    import os
    import statistics

    N = args.batch
    slots = list(range(N))

    def loop(toks):
        for s, t in enumerate(toks):
            eng.prefill_prompt(t, s, 0)

    def packed(flag):
        def run(toks):
            os.environ["MDI_PREFILL_VARLEN_ATTN"] = flag
            eng.prefill_prompts(toks, slots)
        return run

    paths = (("loop", loop), ("packed+loop", packed("0")),
             ("packed+varlen", packed("1")))
    for T in lengths:
        toks = [torch.randint(0, cfg.vocab_size, (T,), device=dev)
                for _ in range(N)]
        for _, fn in paths:
            fn(toks)
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in paths}
        for rnd in range(args.rounds):
            for name, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn(toks)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / args.reps * 1e3)
                print(f"prefill {args.model} {N}x{T} round {rnd} "
                      f"{name:>13}: {ms[name][-1]:9.2f} ms", flush=True)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(f"prefill {args.model} {N}x{T} median ms: "
              + "  ".join(f"{k} {v:.2f}" for k, v in med.items())
              + f"  loop/varlen {med['loop'] / med['packed+varlen']:.2f}x"
              f"  packed-loop/varlen "
              f"{med['packed+loop'] / med['packed+varlen']:.2f}x",
              flush=True)


def main():
    from mdi_llm_amd.config import ModelConfig
    from mdi_llm_amd.models.stages import StarterStage
    from mdi_llm_amd.ops.engine import DecodeEngine

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Meta-Llama-3-8B-Instruct")
    ap.add_argument("--lengths", default="512,2048,4096")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0,
                    help="N prompts of each length, one per slot: the "
                         "per-prompt loop against the packed pass")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    cfg = ModelConfig.from_name(args.model)
    torch.manual_seed(0)
    torch.set_default_dtype(torch.bfloat16)
    with torch.device(dev):
        stage = StarterStage(cfg, cfg.n_layer)
    torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for p in stage.parameters():
            p.normal_(0, 0.02)
    stage.max_seq_length = min(4096, cfg.block_size)
    if args.batch:  # N slots: keep each no longer than the prompts
        stage.max_seq_length = min(
            stage.max_seq_length,
            max(int(t) for t in args.lengths.split(",")))
    stage.eval()
    stage.set_kv_cache(max(1, args.batch))
    eng = DecodeEngine(stage, stage.kv_pool, use_graphs=False)
    assert eng.supports_hip_prefill, f"{args.model}: no HIP prefill"

    lengths = sorted({min(int(t), stage.max_seq_length)
                      for t in args.lengths.split(",")})
    if args.batch:
        return bench_batch(args, cfg, eng, lengths, dev)
    prompts = {T: torch.randint(0, cfg.vocab_size, (T,), device=dev)
               for T in lengths}

    def hip(toks):
        eng.prefill_prompt(toks, 0, 0)

    def ref(toks):
        with torch.inference_mode():
            stage.forward_head(toks.view(1, -1), slot=0, input_pos=0)

    paths = (("hip", hip), ("torch", ref))
    for toks in prompts.values():
        for _, fn in paths:
            fn(toks)
    torch.cuda.synchronize()

    for T, toks in prompts.items():
        ms = {name: [] for name, _ in paths}
        for rnd in range(args.rounds):
            for name, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn(toks)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / args.reps * 1e3)
                print(f"prefill {args.model} T={T:5d} round {rnd} "
                      f"{name:>6}: {ms[name][-1]:8.2f} ms", flush=True)
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / mean[k] for k, v in ms.items()}
        print(f"prefill {args.model} T={T:5d} torch/hip "
              f"{mean['torch'] / mean['hip']:.2f}x  spread hip "
              f"{spread['hip']:.1%} torch {spread['torch']:.1%}", flush=True)


if __name__ == "__main__":
    main()
