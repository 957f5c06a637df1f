"""Word2Vec hierarchical-softmax step: HIP route against the torch route.

A synthetic Zipf corpus (seed and sizes are printed) is trained for one epoch
with skip-gram and CBOW on both routes of ops/w2v_ops.py, alternating, and one
batch of 16384 examples is timed alone (device events) on both routes and on a
few launch plans.  Needs a GPU.

    python scripts/w2v_mb.py --tokens 10000000 --vocab 100000 --repeats 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
import h2o3_amd as h2o                                            # noqa: E402
from h2o3_amd.core.frame import H2OFrame                         # noqa: E402
from h2o3_amd.core.vec import make_enum                          # noqa: E402
from h2o3_amd.estimators import H2OWord2vecEstimator             # noqa: E402
from h2o3_amd.models.word2vec import _huffman                    # noqa: E402
from h2o3_amd.ops import w2v_ops                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=1_000_000)
ap.add_argument("--vocab", type=int, default=10_000)
ap.add_argument("--d", type=int, default=100)
ap.add_argument("--window", type=int, default=5)
ap.add_argument("--sentence", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--batch-iters", type=int, default=30)
ap.add_argument("--skip-train", action="store_true")
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("w2v_mb.py measures on a GPU; none found")
h2o.init(verbose=False)
dev = torch.device("cuda")
print(json.dumps({"shape": vars(a), "device": torch.cuda.get_device_name(0)}), flush=True)

rng = np.random.default_rng(a.seed)
p = 1.0 / (1 + np.arange(a.vocab))
p /= p.sum()
ids = rng.choice(a.vocab, size=a.tokens, p=p).astype(np.int32)


def step_time(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


# ---- one batch alone: the three kernels (+ counter memset) against the torch rule
counts = np.bincount(ids, minlength=a.vocab)
order = np.argsort(-counts, kind="stable")
counts = counts[order][counts[order] > 0]
V = len(counts)
rank_of = np.empty(a.vocab, dtype=np.int64)
rank_of[order] = np.arange(a.vocab)
tb = w2v_ops.HuffmanTables(*_huffman(counts), dev)
g = torch.Generator().manual_seed(a.seed)
B, W = 16384, 2 * a.window
words = torch.from_numpy(rank_of[ids[:B * (W + 1)]]).to(dev)
c, ctx = words[:B].contiguous(), words[B:].view(B, W).contiguous()
mask = (torch.rand((B, W), generator=g) < 0.6).to(dev)
syn0 = ((torch.rand((V, a.d), generator=g) - 0.5) / a.d).to(dev)
syn1 = (torch.randn((tb.nodes, a.d), generator=g) * 0.1).to(dev)
sc = w2v_ops.Scratch(B, a.d, tb, dev)
cus = torch.cuda.get_device_properties(dev).multi_processor_count
for name, w_in, m in (("skipgram", ctx[:, 0].contiguous(), None), ("cbow", ctx, mask)):
    row = {"batch": name, "B": B, "V": V, "L": tb.L, "d": a.d}
    for threads in (256, 512):
        for per_cu in (1, 2, 4):
            plan = (None, threads, per_cu * cus)
            row[f"hip_ms_t{threads}_g{per_cu}cu"] = round(step_time(
                lambda: w2v_ops.hsm_step(syn0, syn1, tb, c, w_in, m, 1e-4, sc, plan), a.batch_iters), 4)
    row["hip_ms_default"] = round(step_time(lambda: w2v_ops.hsm_step(syn0, syn1, tb, c, w_in, m, 1e-4, sc),
                                            a.batch_iters), 4)
    row["hip_ms_no_cache"] = round(step_time(
        lambda: w2v_ops.hsm_step(syn0, syn1, tb, c, w_in, m, 1e-4, sc, (0,)), a.batch_iters), 4)
    row["torch_ms"] = round(step_time(lambda: w2v_ops.hsm_step_torch(syn0, syn1, tb, c, w_in, m, 1e-4),
                                      a.batch_iters), 4)
    print(json.dumps(row), flush=True)
del syn0, syn1, sc, words, c, ctx, mask

# ---- train(): one epoch, both routes alternating
if not a.skip_train:
    codes = ids.copy()
    codes[a.sentence - 1::a.sentence] = -1                 # NA = sentence break
    fr = H2OFrame.from_vecs([make_enum(codes, [f"w{i}" for i in range(a.vocab)])], ["w"])
    n_tok = int((codes >= 0).sum())
    for wm in ("SkipGram", "CBOW"):
        for rep in range(a.repeats):
            for route in ("hip", "torch"):
                os.environ["H2O3_W2V"] = route
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                m = H2OWord2vecEstimator(vec_size=a.d, window_size=a.window, epochs=1, min_word_freq=1, seed=a.seed,
                                         word_model=wm)
                m.train(training_frame=fr)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                loop = m._output["w2v_loop_seconds"]
                assert m._output["w2v_route"] == route
                print(json.dumps({"train": wm, "route": route, "rep": rep, "tokens": n_tok, "train_s": round(dt, 3),
                                  "loop_s": round(loop, 3), "tokens_per_s_train": round(n_tok / dt),
                                  "tokens_per_s_loop": round(n_tok / loop),
                                  "peak_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                                  "finite": bool(torch.isfinite(m._vecs).all())}), flush=True)
                del m
