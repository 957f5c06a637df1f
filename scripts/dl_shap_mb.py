"""Microbenchmark of the DeepSHAP pair kernel (ops/csrc/dl_shap.hip) against
the torch rule on the same GPU.

    python scripts/dl_shap_mb.py [--reps 5] [--out profiles/dl_shap_mb.txt]

Two shapes, 100 inputs, hidden [200, 200], rectifier: 10k test rows x 100
background rows, and 1 test row x 10k background rows.  Each timing is the
median of --reps calls of deep_shap (forward of both frames + pair stage +
averaging), after one warm-up call, with a device synchronise inside the
timed window; the two implementations alternate.  The results are compared at
the timed size before any time is printed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from h2o3_amd.ops import dl_shap_ops  # noqa: E402

SHAPES = [(10000, 100), (1, 10000)]
WIDTHS = [100, 200, 200, 1]


def net(act, dev):
    g = torch.Generator().manual_seed(1)
    layers = []
    for fin, fout in zip(WIDTHS[:-2], WIDTHS[1:-1]):
        layers.append(((torch.randn((fout, fin), generator=g) / fin ** 0.5).to(dev),
                       (torch.randn(fout, generator=g) * 0.3).to(dev)))
    return layers, [act] * len(layers), [0.9] * len(layers), torch.randn(WIDTHS[-2], generator=g).to(dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--act", default="rectifier")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dl_shap_mb needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lines = [f"# dl_shap_mb: widths {WIDTHS}, {a.act}, median of {a.reps} calls (ms), {torch.cuda.get_device_name(0)}"]
    layers, acts, scales, out_w = net(a.act, dev)
    for N, B in SHAPES:
        g = torch.Generator().manual_seed(N + B)
        X = torch.randn((N, WIDTHS[0]), generator=g).to(dev)
        Z = torch.randn((B, WIDTHS[0]), generator=g).to(dev)
        kern = lambda: dl_shap_ops.deep_shap(layers, acts, scales, out_w, X, Z, use_native=True)
        rule = lambda: dl_shap_ops.deep_shap(layers, acts, scales, out_w, X, Z, use_native=False)
        _, rk = timed(kern)
        _, rt = timed(rule)
        assert rk.kernel and not rt.kernel
        diff = float((rk.phi - rt.phi).abs().max())
        top = float(rt.phi.abs().max())
        tk, tt = [], []
        for _ in range(a.reps):
            tk.append(timed(kern)[0])
            tt.append(timed(rule)[0])
        pairs = {}
        dl_shap_ops.deep_shap(layers, acts, scales, out_w, X, Z, use_native=True, timing=pairs)
        mk, mt = statistics.median(tk), statistics.median(tt)
        flop = 2.0 * N * B * sum(i * o for i, o in zip(WIDTHS[:-2], WIDTHS[1:-1]))
        lines.append(f"N={N} B={B}: kernel {mk:.2f} ms (min {min(tk):.2f}, max {max(tk):.2f}; pair stage "
                     f"{pairs['pairs_ms']:.2f} ms, {flop / pairs['pairs_ms'] / 1e9:.2f} TFLOP/s of its "
                     f"{flop / 1e12:.3f} TFLOP), torch rule {mt:.2f} ms (min {min(tt):.2f}, max {max(tt):.2f}), "
                     f"ratio {mt / mk:.2f}x; max |kernel - torch rule| {diff:.3e} at max |phi| {top:.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
