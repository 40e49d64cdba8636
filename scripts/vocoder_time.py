"""Device time of the generator alone on one 30 s 48 kHz v2 clip for the three decoders (Default NSF-HiFiGAN,
MRF-HiFi-GAN, RefineGAN; synthetic weights), and of the kernels only the new decoders use (csrc/vocoder.hip) at the
shapes the generator launches them with.  Idle GPU, warm-up, HIP events around each call, median of --reps.

For rvc_upsample_linear and rvc_adain the achieved bytes/s (bytes read + bytes written) stands against a torch
device-to-device ``copy_`` moving the same number of bytes, measured in the same process.

    python scripts/vocoder_time.py [--frames 3000] [--reps 20] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rvc-maker_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from rvc_amd import ops, synth, synthetic
    T, dev = a.frames, "cuda"

    def timed(fn):
        ts = []
        for _ in range(a.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[3:])
        return ts[len(ts) // 2]

    def copy_rate(nbytes):
        """GB/s (read + write) of a device-to-device copy_ moving ``nbytes`` in all: nbytes/2 read, nbytes/2 written."""
        n = max(nbytes // 8, 1)
        src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
        return nbytes / (timed(lambda: dst.copy_(src)) * 1e-3) / 1e9

    out = {"frames": T, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator().manual_seed(0)
    nsff0 = (torch.rand(1, T, generator=g) * 300 + 80)
    nsff0[:, T // 3: T // 3 + 200] = 0
    nsff0 = nsff0.to(dev)
    for vocoder in ("Default", "MRF-HiFi-GAN", "RefineGAN"):
        m = synth.SynthesizerAMD(synthetic.make_synth_ckpt(48000, "v2", seed=7, vocoder=vocoder), dev)
        gc = m.speaker_cond(0)
        z = torch.randn(1, m.inter, T, device=dev)
        L = T * m.upp
        r = {}
        if m.kind == "nsf":
            noise = torch.randn(1, L, device=dev)
            r["generator_ms"] = timed(lambda: m.generator(z, nsff0, gc[4 * 6 * m.hidden:], T, noise, 1))
        else:
            # the production form: every draw made on the device from the seed, as decode_batch does it
            r["generator_ms"] = timed(lambda: m.decode_batch(z, nsff0, gc, None, (3,)))
            H = m.n_harm
            noise = torch.randn(1, L, H, device=dev)
            ph = torch.zeros(1, H, device=dev)
            r["harmonic_source_ms"] = timed(lambda: m.harmonic_source(nsff0, noise, ph, T, 1))
            r["source_noise_draw_ms"] = timed(lambda: ops.randn(noise, 3, ops.OFF_SINE))
        if m.kind == "refinegan":
            Lc, ups, ada = T, [], []
            for st in m.rg_stages:
                rate, cin, C = st["rate"], st["cin"], st["cout"]
                Lo = Lc * rate
                ccat = cin + cin // 4
                x = torch.randn(1, cin, Lc, device=dev)
                cat = torch.empty(1, ccat, Lo, device=dev)
                ms = timed(lambda: ops.upsample_linear(x, rate, out=cat, act=ops.ACT_LRELU, slope=0.2,
                                                       y_bstride=ccat * Lo))
                nbytes = 4 * cin * (Lc + Lo)
                ups.append(dict(C=cin, Lin=Lc, rate=rate, ms=ms, GBps=nbytes / (ms * 1e-3) / 1e9,
                                copy_GBps=copy_rate(nbytes)))
                del x, cat
                xin = torch.randn(1, C, Lo, device=dev)
                y = torch.empty(1, C, Lo, device=dev)
                w = st["branches"][0][1]
                ms_in = timed(lambda: ops.adain(xin, w, y, seeds=(3,), offset=ops.off_adain(0), slope=0.2))
                ms_acc = timed(lambda: ops.adain(xin, w, y, seeds=(3,), offset=ops.off_adain(1), slope=0.2,
                                                 out_scale=1 / 3, accumulate=True))
                nb_in, nb_acc = 4 * C * Lo * 2, 4 * C * Lo * 3
                ada.append(dict(C=C, L=Lo, ms=ms_in, GBps=nb_in / (ms_in * 1e-3) / 1e9, copy_GBps=copy_rate(nb_in),
                                accumulate_ms=ms_acc, accumulate_GBps=nb_acc / (ms_acc * 1e-3) / 1e9,
                                accumulate_copy_GBps=copy_rate(nb_acc)))
                del xin, y
                Lc = Lo
            r["upsample_linear"], r["adain"] = ups, ada
            r["upsample_linear_total_ms"] = sum(u["ms"] for u in ups)
            # per stage: three leading AdaINs, one trailing one that writes and two that accumulate
            r["adain_total_ms"] = sum(4 * s["ms"] + 2 * s["accumulate_ms"] for s in ada)
        out[vocoder] = r
        print(f"{vocoder:14s} generator {r['generator_ms']:8.3f} ms per {T / 100:.0f} s clip" +
              "".join(f"  {k[:-3]} {v:.3f} ms" for k, v in r.items() if k.endswith("_ms") and k != "generator_ms"),
              flush=True)
        for kind in ("upsample_linear", "adain"):
            for s in r.get(kind, []):
                shape = (f"C={s['C']:3d} Lin={s['Lin']:7d} r={s['rate']:2d}" if "rate" in s else
                         f"C={s['C']:3d} L={s['L']:8d}      ")
                line = f"  {kind:16s} {shape}  {s['ms']:.3f} ms  {s['GBps']:7.1f} GB/s  copy_ {s['copy_GBps']:7.1f} GB/s"
                if "accumulate_ms" in s:
                    line += (f"   accumulate {s['accumulate_ms']:.3f} ms  {s['accumulate_GBps']:7.1f} GB/s  "
                             f"copy_ {s['accumulate_copy_GBps']:7.1f} GB/s")
                print(line, flush=True)
        del m
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
