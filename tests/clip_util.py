"""The float64 reference of nr_grad_norm_multi (include/newsrec_hip.h) and helpers shared by
tests/test_clip_cpu.py and tests/test_clip_gpu.py.

Tolerance.  The kernel accumulates the squares in double, so against this reference the only
error of ``norm`` is the final rounding to float (6e-8 relative); an fp32 tree of depth <= 24 over
non-negative terms would be bounded by 24 * 2^-24 = 1.4e-6 on the sum, 0.7e-6 on its square root.
RTOL = 1e-6 holds either; with the tests' shapes one dropped 4096-element chunk is an error of 1e-3
or more."""
import numpy as np

RTOL = 1e-6
CHUNK = 4096   # elements per partial (Adam's kAdamChunk)


def norm_ref(grads, grad_scale=1.0):
    """|grad_scale| * sqrt(sum float64(g)^2) over numpy arrays / CPU or CUDA tensors."""
    s = 0.0
    for g in grads:
        a = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
        a = a.astype(np.float64).ravel()
        s += float(np.dot(a, a))
    return abs(float(grad_scale)) * float(np.sqrt(s))


def scale_ref(norm, grad_scale, max_norm):
    """The scale the library forms from the float32 ``norm`` it stored (float64 arithmetic)."""
    with np.errstate(all="ignore"):
        coef = np.float64(max_norm) / (np.float64(np.float32(norm)) + 1e-6)
        clamped = np.float64(1.0) if coef > 1.0 else coef
        return float(np.float64(np.float32(grad_scale)) * clamped)


def clips(norm, max_norm):
    return float(max_norm) / (float(np.float32(norm)) + 1e-6) <= 1.0


def workspace_floor(sizes):
    """Bytes of one double per 4096-element chunk of every tensor."""
    return 8 * sum((int(n) + CHUNK - 1) // CHUNK for n in sizes)


def read_state(state):
    """The 16 state bytes -> {"norm", "scale", "nonfinite", "nonfinite_total"} (synchronises)."""
    import torch
    w = state.view(torch.int32).cpu()
    f = w.view(torch.float32)
    return {"norm": float(f[0]), "scale": float(f[1]), "nonfinite": int(w[2]), "nonfinite_total": int(w[3])}


def close(got, want, rtol=RTOL):
    return abs(got - want) <= rtol * abs(want)
