"""Eager HIP-event timing of the retrieval scorer with and without the chunk-mean index at the
configs[1] shape (7B: 32 heads, head_dim 128, 15 616 chunks of 8 rows): tf_retrieval_score over K, tf_retrieval_score_indexed
over the index, tf_chunk_mean over the few new chunks of a re-anchor and over all of them (the first build).  L2 flushed in
front of every launch, median of --iters; the two scorers' outputs are compared bit for bit on the way.  One JSON line per
kernel on stdout.

    python tools/reanchor_bench.py [--iters 50] [--out profiles/...jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triforce_amd import ops  # noqa: E402


def timed(fn, iters, flush):
    ts = []
    for _ in range(iters):
        flush.zero_()                                    # evict: every launch streams its input from HBM
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--chunks", type=int, default=15616)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--new-chunks", type=int, default=8, help="chunks a re-anchor adds to the index")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, D, H, C, chunk, new = "cuda:0", 128, args.heads, args.chunks, args.chunk, args.new_chunks
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    k = torch.randn(H, (C + new) * chunk, D, device=dev).half()
    q = torch.randn(H, D, device=dev).half()
    index = torch.zeros(H, C + new, D, dtype=torch.float16, device=dev)
    ops.chunk_mean(k, index, 0, C + new, chunk)
    same = torch.equal(ops.retrieval_score_indexed(index, q, C).view(torch.int16), ops.retrieval_score(k, q, C, chunk).view(torch.int16))
    t_score = timed(lambda: ops.retrieval_score(k, q, C, chunk), args.iters, flush)
    t_indexed = timed(lambda: ops.retrieval_score_indexed(index, q, C), args.iters, flush)
    t_new = timed(lambda: ops.chunk_mean(k, index, C, C + new, chunk), args.iters, flush)
    t_all = timed(lambda: ops.chunk_mean(k, index, 0, C, chunk), args.iters, flush)
    kb, ib = H * C * chunk * D * 2, H * C * D * 2
    shape = {"H": H, "C": C, "chunk": chunk, "D": D, "iters": args.iters}
    rows = [
        dict(shape, kernel="tf_retrieval_score", us=round(t_score, 1), bytes_read=kb, TBps=round(kb / t_score / 1e6, 2)),
        dict(shape, kernel="tf_retrieval_score_indexed", us=round(t_indexed, 1), bytes_read=ib, TBps=round(ib / t_indexed / 1e6, 2),
             over_tf_retrieval_score=round(t_indexed / t_score, 3), byte_model=round(ib / kb, 3), bit_identical=same),
        dict(shape, kernel="tf_chunk_mean", chunks=new, us=round(t_new, 1)),
        dict(shape, kernel="tf_chunk_mean", chunks=C, us=round(t_all, 1), bytes_read=kb, TBps=round(kb / t_all / 1e6, 2)),
    ]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not same:
        raise SystemExit("tf_retrieval_score_indexed differs from tf_retrieval_score")


if __name__ == "__main__":
    main()
