"""Times global-norm gradient clipping on the NRMS parameter set (the 30522 x 768 word table + ~1.2 M
dense parameters in 20 tensors, 24.6 M elements; the word table's gradient row-sparse, its touched
rows those of one formed bench batch):

  (a) FusedAdam.step()                                   unclipped
  (b) FusedAdam(max_grad_norm=2.0).step()                the built-in clip
  (b') the same with the norm pass's loads plain, not    (the --build-plain library, when built)
       nontemporal
  (c) torch.nn.utils.clip_grad_norm_(params, 2.0), (a)   what a user had to do before (it rewrites
                                                         every .grad, so the row flags are dropped)

each on its own parameters, gradients and moments, alternating in one process: eager (host clock
around N steps ending in a synchronise) and as replays of a captured graph (device time without the
host).  Then the norm call alone (nr_grad_norm_multi: the partial launches plus the one-workgroup
finish) with and without row flags, with nontemporal (the product) and with plain loads, warm
(repeated over the same 98 MB, which fit the Infinity Cache) and cold (a 1 GiB fill between calls),
with the bytes it reads and the fraction of the 6.29 TB/s measured copy rate.  Prints one JSON line.

The plain-loads build is a second library with csrc/score_adam.hip compiled
-DNR_GRAD_NORM_PLAIN_LOADS:
  python tools/clip_probe.py --build-plain  (no GPU needed)
  python tools/clip_probe.py [--rounds 7] [--steps 20]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "news-recommendation-mind_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
ALT_LIB = os.path.join(PKG, "newsrec_amd", "lib", "libnr_clip_probe_plain.so")
COPY_RATE = 6.29e12   # B/s, the measured device copy rate


def build_plain():
    """The whole library with score_adam.hip compiled -DNR_GRAD_NORM_PLAIN_LOADS (the other objects are the
    in-tree build's; run build() first)."""
    import glob
    import build as B
    B.build(verbose=False)
    obj = os.path.join(B.OUT, "obj", "score_adam_plain_loads.o")
    src = os.path.join(B.CSRC, "score_adam.hip")
    subprocess.run([B.HIPCC] + B.FLAGS + ["-DNR_GRAD_NORM_PLAIN_LOADS=1", "-c", src, "-o", obj], check=True)
    rest = [o for o in glob.glob(os.path.join(B.OUT, "obj", "*.hip.*.o")) if "score_adam.hip." not in o]
    rest.append(os.path.join(B.OUT, "obj", "version.o"))
    subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", ALT_LIB, obj] + rest, check=True)
    print("built", ALT_LIB)


def med(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-plain", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.build_plain:
        return build_plain()

    import torch
    import bench
    from newsrec_amd import _lib as L, kernels as K
    from newsrec_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    V, E = bench.V, bench.E
    shapes = [(V, E), (1152, 768), (1152,), (384,), (384,), (384,), (768, 384), (768,), (384,)]
    shapes += [(384, 384)] * 2 + [(384,)] * 9
    n = sum(int(torch.Size(s).numel()) for s in shapes)

    # the word table's touched rows: the distinct token ids of one formed bench batch
    x = bench.synth_batch(torch.Generator().manual_seed(0), dev)
    ids = torch.cat([x["cdd_encoded_index"].reshape(-1), x["his_encoded_index"].reshape(-1)]).unique()
    ids = ids[ids != 0]
    flags = torch.zeros(V, dtype=torch.uint8, device=dev)
    flags[ids] = 1
    touched = int(flags.sum())
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(s, device=dev, generator=gen) * 1e-2 for s in shapes]
    grads[0] *= flags[:, None].float()

    alt = None
    if os.path.exists(ALT_LIB):
        alt = ctypes.CDLL(ALT_LIB)
        for name, argtypes in L._SIGS.items():
            getattr(alt, name).argtypes = argtypes
            getattr(alt, name).restype = L._RESTYPES.get(name, ctypes.c_int32)
    prod = L.load()

    def variant(**kw):
        ps = [torch.randn(s, device=dev, generator=gen).requires_grad_(True) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        ps[0]._nr_row_touched = (ps[0].grad, flags, ps[0].grad._version)
        return ps, FusedAdam(ps, lr=1e-4, **kw)

    def steps_of(capturable):
        out = {}
        for name, kw, clip_first, lib in (("a_unclipped", {}, False, prod),
                                          ("b_clipped", {"max_grad_norm": 2.0}, False, prod),
                                          ("b_clipped_plain_loads", {"max_grad_norm": 2.0}, False, alt),
                                          ("c_torch_clip", {}, True, prod)):
            if lib is None:
                continue
            ps, opt = variant(capturable=capturable, **kw)

            def step(ps=ps, opt=opt, clip_first=clip_first, lib=lib):
                if clip_first:
                    torch.nn.utils.clip_grad_norm_(ps, 2.0)
                L._lib = lib            # (the binding's loaded library: the plain-loads build for b')
                try:
                    opt.step()
                finally:
                    L._lib = prod
            out[name] = step
        return out

    def time_rounds(fns, reps):
        """Per variant, the per-call time in us of each round (variants alternate within a round)."""
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        res = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                torch.cuda.synchronize()
                res[k].append((time.perf_counter() - t0) * 1e6 / reps)
        return res

    out = {"elements": n, "table_rows_touched": touched, "table_rows": V, "rounds": a.rounds, "steps": a.steps}
    eager = time_rounds(steps_of(False), a.steps)
    out["eager_us"] = {k: med(v) for k, v in eager.items()}

    graphed = {}
    for k, f in steps_of(True).items():
        try:
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                f()
            graphed[k] = g.replay
        except Exception as e:   # (reported, not hidden: the variant has no graphed time)
            out.setdefault("graph_errors", {})[k] = repr(e)[:200]
    if graphed:
        out["graph_us"] = {k: med(v) for k, v in time_rounds(graphed, a.steps).items()}
    for key in ("eager_us", "graph_us"):
        t = out.get(key, {})
        if all(k in t for k in ("a_unclipped", "b_clipped", "c_torch_clip")):
            t["b_minus_a"] = round(t["b_clipped"]["median"] - t["a_unclipped"]["median"], 2)
            t["c_minus_a"] = round(t["c_torch_clip"]["median"] - t["a_unclipped"]["median"], 2)
            if "b_clipped_plain_loads" in t:
                t["b_plain_loads_minus_a"] = round(t["b_clipped_plain_loads"]["median"] -
                                                   t["a_unclipped"]["median"], 2)

    # the norm call alone
    libs = {"nontemporal": prod}
    if alt is not None:
        libs["plain"] = alt
    else:
        out["plain"] = "not built (python tools/clip_probe.py --build-plain)"
    ents = {"flags": [(g, g, g, g, 1e-4, 1) + ((flags,) if i == 0 else ()) for i, g in enumerate(grads)],
            "dense": [(g, g, g, g, 1e-4, 1) for g in grads]}
    nbytes = {"dense": 4 * n, "flags": 4 * (n - (V - touched) * E) + V}
    state = K.clip_state(dev)
    K.grad_norm_multi(ents["dense"], 1.0, 2.0, state)       # creates the workspace
    work = K.self_cleaning_workspace(dev, "nr_grad_norm_multi", 0, clean=[])
    calls = {}
    for lname, lib in libs.items():
        for ename, ent in ents.items():
            arr = K._adam_descriptors(ent)

            def call(lib=lib, arr=arr, cnt=len(ent)):
                rc = lib.nr_grad_norm_multi(arr, cnt, 1.0, 2.0, L.ptr(work), work.numel() * 4, L.ptr(state),
                                            L.stream_ptr(state))
                assert rc == 0, rc
            calls[lname + "/" + ename] = call
    norms = {}
    for k, f in calls.items():
        f()
        norms[k] = state.view(torch.float32)[0].item()
    assert len(set(norms.values())) == 1, norms              # same bits from every variant
    warm = time_rounds(calls, 50)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    cold = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, f in calls.items():
            flush.fill_(1.0)
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            cold[k].append(ev[0].elapsed_time(ev[1]) * 1e3)
    out["norm_call"] = {}
    for k in calls:
        b = nbytes[k.split("/")[1]]
        w, c = med(warm[k]), med(cold[k])
        out["norm_call"][k] = {"bytes": b, "warm_us": w, "cold_us": c,
                               "warm_frac_of_copy_rate": round(b / (w["median"] * 1e-6) / COPY_RATE, 3),
                               "cold_frac_of_copy_rate": round(b / (c["median"] * 1e-6) / COPY_RATE, 3)}
    out["norm"] = norms["nontemporal/dense"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
