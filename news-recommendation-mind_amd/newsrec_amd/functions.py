"""autograd.Functions over the HIP kernels — the fused hot path of the two towers.

Every forward/backward here launches only libnewsrec_hip.so kernels (plus torch allocations
and zero-fills); nothing computes on the CPU.  Token ids are int64 [T] (T = news * L), masks
are passed in their reference dtype (i64 token masks, f64 history masks).

News towers read the word-embedding table directly (the gather is fused into the first GEMM's
operand loader) and scatter the table gradient straight out of the dgrad GEMM, so the
[T, 768] embedding activations are never materialised.  A standalone ``encoderN(emb, mask)``
call uses the same functions with the embeddings as the "table" and identity row ids.
"""
import functools
import os
import threading
import weakref

import torch

from . import _lib as L
from . import kernels as K


def _gemm_backward(fn):
    """Run a Function's backward under the GEMM arithmetic its forward recorded in ``ctx.prec``
    (the autograd engine runs CUDA backwards on its own thread, which has its own default)."""
    @functools.wraps(fn)
    def wrapper(ctx, *grads):
        with K.gemm_precision(ctx.prec):
            return fn(ctx, *grads)
    return wrapper


def _ceil32(n):
    return (n + 31) // 32 * 32


def _pad4(n):
    return (n + 3) // 4 * 4


def _empty(rows, cols, like, ld=None):
    """[rows, cols] view of a row-major buffer with a float4-friendly leading dimension."""
    ld = _pad4(cols) if ld is None else ld
    buf = torch.empty(rows, ld, device=like.device, dtype=torch.float32)
    return buf[:, :cols]


GRAD_COPIES = 32
_GRAD_COPIES_WS = {}


def _grad_copies(dev, width):
    """A persistent zeroed [GRAD_COPIES, ceil4(width)] workspace per (device, width) for
    nr_mha_pool_bwd's spread parameter-gradient atomics (the kernel leaves it zero again).

    Created eagerly, never inside a graph capture: a buffer first allocated (and zero-filled) during
    a capture would only be zero once that graph had replayed, and a later graph reusing it would
    depend on that replay order.  Steps run one at a time on a device, so one workspace per
    (device, width) serves every stream."""
    key = (torch.device(dev), width)
    ws = _GRAD_COPIES_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise L.HipError("nr_mha_pool_bwd workspace must be created by an eager step before graph capture")
        ws = _GRAD_COPIES_WS[key] = torch.zeros(GRAD_COPIES, (width + 3) // 4 * 4, device=dev)
    return ws


def _zeros_views(dev, *shapes):
    """Views of ONE zero-filled buffer (one fill launch instead of one per gradient), each
    starting 16-B aligned."""
    sizes = [int(torch.Size(sh).numel()) for sh in shapes]
    offs, tot = [], 0
    for n in sizes:
        offs.append(tot)
        tot += _pad4(n)
    buf = torch.zeros(max(tot, 1), device=dev)
    return [buf[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, shapes)]


class _ZeroArena:
    """One zero fill for the small zero-initialised gradients of a training step.

    A Function's forward reserves the shapes its backward will zero-fill (``reserve``, only when a
    backward can run); the first backward that takes its views (``take``) zero-fills every
    reservation made since the previous fill with ONE launch.  The NRMS step had three such fills
    (the news tower's five parameter gradients, the user encoder's two, the pooling query's), each a
    launch of its own in the graph.  A token is taken once: a second backward over the same graph
    (retain_graph) gets fresh zeros, as do reservations past LIMIT floats."""

    LIMIT = 8 << 20

    def __init__(self):
        self.cur = None

    def reserve(self, dev, *shapes):
        sizes = [int(torch.Size(sh).numel()) for sh in shapes]
        need = sum(_pad4(n) for n in sizes)
        a = self.cur
        if a is None or a["buf"] is not None or a["dev"] != dev or a["tot"] + need > self.LIMIT:
            a = self.cur = {"dev": dev, "tot": 0, "buf": None}
        offs = []
        for n in sizes:
            offs.append(a["tot"])
            a["tot"] += _pad4(n)
        return {"arena": a, "offs": offs, "sizes": sizes, "shapes": shapes, "taken": False}

    def take(self, tok, dev, *shapes):
        """The reserved views (zero), or ``_zeros_views(dev, *shapes)`` without a usable token."""
        if tok is None or tok["taken"] or tuple(tok["shapes"]) != tuple(shapes):
            return _zeros_views(dev, *shapes)
        tok["taken"] = True
        a = tok["arena"]
        if a["buf"] is None:
            a["buf"] = torch.zeros(max(a["tot"], 1), device=a["dev"])
            if self.cur is a:
                self.cur = None
        buf = a["buf"]
        return [buf[o:o + n].view(sh) for o, n, sh in zip(tok["offs"], tok["sizes"], shapes)]


ZERO_ARENA = _ZeroArena()


_CALLER_GRAD = threading.local()


class _GradAwareFn(torch.autograd.Function):
    """A Function whose forward may ask ``_backward_possible``: torch runs forward() with grad mode
    OFF whatever the caller's mode, so apply() records the caller's mode for it (per thread, restored
    on exit, so nested applies see their own caller's)."""

    @classmethod
    def apply(cls, *args, **kwargs):
        prev = getattr(_CALLER_GRAD, "on", None)
        _CALLER_GRAD.on = torch.is_grad_enabled()
        try:
            return super().apply(*args, **kwargs)
        finally:
            _CALLER_GRAD.on = prev


def _backward_possible(ctx):
    """A backward can follow this forward (of a _GradAwareFn): its caller had autograd recording (not
    torch.no_grad(), where needs_input_grad still reports the parameters' requires_grad) and some input
    wants a gradient."""
    on = getattr(_CALLER_GRAD, "on", None)
    if on is None:
        raise RuntimeError("_backward_possible needs a _GradAwareFn forward")
    return on and any(ctx.needs_input_grad)


def _reserve_zeros(ctx, dev, *shapes):
    """Forward side of ZERO_ARENA: reserve the backward's zero-initialised gradients (when one can run)."""
    ctx.zero_tok = ZERO_ARENA.reserve(dev, *shapes) if _backward_possible(ctx) else None


def _backward_zeros(ctx, dev, *shapes):
    return ZERO_ARENA.take(getattr(ctx, "zero_tok", None), dev, *shapes)


class _GradDest:
    """Where a consumer's backward may write the gradient of one of its inputs directly: SplitRowsFn
    offers the two halves of its joined gradient buffer for its two outputs; a consumer Function
    (scorer, user encoder) that takes the offer in its forward stores its input gradient there, and
    SplitRowsFn's backward then finds both halves in place and skips the join copy.  The written
    values are that consumer's true gradient either way, so a stale or unused offer costs nothing
    but the copy it fails to save."""

    def __init__(self):
        self.offers = {}

    @staticmethod
    def _key(t):
        return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.device)

    def offer(self, t, dest):
        self.offers[self._key(t)] = dest

    def clear(self):
        self.offers.clear()

    def take(self, t):
        if not self.offers:
            return None
        d = self.offers.pop(self._key(t), None)
        if d is None or d.shape != t.shape:
            return None
        return d


GRAD_DEST = _GradDest()


def _grad_out(dest, rows, cols, like):
    """The backward's output buffer for an input gradient: the offered destination or a new one."""
    if dest is not None:
        return dest
    return _empty(rows, cols, like)


class SplitRowsFn(torch.autograd.Function):
    """``torch.split(x, [n0, rows - n0])`` of a row-major [rows, H] activation (the joint news-encoder
    output -> candidates | history).  torch's backward joins the two gradients with a copy (a cat);
    here the joined gradient buffer is allocated in the forward and its halves offered (GRAD_DEST) to
    the Functions that consume the two outputs, so the join is free when both write in place."""

    stats = {"in_place": 0, "copied": 0}   # backward joins by path (tests)

    @staticmethod
    def forward(ctx, x, n0):
        rows, H = x.shape
        g = _empty(rows, H, x)
        a, b = x[:n0], x[n0:]
        GRAD_DEST.clear()
        GRAD_DEST.offer(a, g[:n0])
        GRAD_DEST.offer(b, g[n0:])
        ctx.g, ctx.n0 = g, n0
        return a, b

    @staticmethod
    def backward(ctx, da, db):
        g, n0 = ctx.g, ctx.n0
        ga, gb = g[:n0], g[n0:]
        if (da is not None and db is not None and da.data_ptr() == ga.data_ptr() and
                db.data_ptr() == gb.data_ptr() and da.stride() == ga.stride() and db.stride() == gb.stride()):
            SplitRowsFn.stats["in_place"] += 1
            return g, None
        SplitRowsFn.stats["copied"] += 1
        out = torch.empty_like(g)
        for d, o in ((da, out[:n0]), (db, out[n0:])):
            if d is None:
                o.zero_()
            else:
                o.copy_(d)
        return out, None


def _split_k(m, n, k, slots=512):
    """Split-K factor for a wgrad GEMM: fill the 256 CUs x 2 resident 128x128 blocks in ONE
    wave (a 1.16-wave grid runs as two), keeping >= 512 k per split."""
    tiles = max(1, ((m + 127) // 128) * ((n + 127) // 128))
    return int(max(1, min(64, slots // tiles, k // 512)))


def _proj_wgrad(dY, X_op, dW, db, M_rows):
    """dW[n_out, k_in] += dYᵀ X ; db += colsum(dY).  dY: [rows, n_out] view, X_op: operand of
    the layer input with MN-contiguous layout (rows = token index)."""
    n_out = dW.shape[0]
    k_in = dW.shape[1]
    # db folds into the GEMM on its split-K workspace path (the first column tile's units sum the dY
    # tiles they load); other routings leave it to the two-pass column sum
    folded = K.gemm(n_out, k_in, M_rows, K.operand(dY, L.MNCONTIG), X_op, dW, epilogue=L.EPI_ATOMIC,
                    split_k=_split_k(n_out, k_in, M_rows), colsum=db)
    if db is not None and not folded:
        K.colsum(dY, M_rows, n_out, db)


class _Probe:
    """Per-launch timing of the step's dominant kernels (the news tower's three projection GEMMs).

    While enabled, ``run(name, fn, out, ur)`` launches ``fn`` as usual and keeps the first launch of
    each name as a closure over its real operands.  ``time()`` then replays every kept closure
    ``reps`` times, each replay bracketed by HIP events on the launch stream and preceded by a 512 MB
    write that evicts the L2s and the Infinity Cache (in the step the operands arrive cold: Adam has
    just streamed 0.7 GB; back-to-back replays with warm operands ran ~8 % faster than the graphed
    step's launches), and restores the output it overwrote: the average per-launch duration of
    exactly the kernels the step runs, free of the eager step's host gaps.  A closure is the whole
    unit of work (the weight gradient = its split-K GEMM + the ordered reduction)."""

    def __init__(self):
        self.on = False
        self.launches = {}

    def enable(self):
        self.on, self.launches = True, {}

    def disable(self):
        self.on, self.launches = False, {}

    def run(self, name, fn, out, ur=None):
        """``fn()`` launches the kernel(s) writing ``out``; ``ur``: the launch's UniqueRows (its
        device-side row count, the GEMM's M or K, is read back at time() for the FLOP count)."""
        fn()
        if self.on and name not in self.launches:
            self.launches[name] = (fn, out, ur)

    def time(self, reps=20, warm=2):
        res = {}
        flush = None
        for name, (fn, out, ur) in self.launches.items():
            if flush is None:
                flush = torch.empty(128 << 20, device=out.device)
            saved = out.clone()
            for _ in range(warm):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for s, e in ev:
                flush.zero_()
                s.record()
                fn()
                e.record()
            torch.cuda.synchronize()
            out.copy_(saved)
            res[name + "_ms"] = sum(s.elapsed_time(e) for s, e in ev) / reps
            if ur is not None:
                res[name + "_rows"] = int(ur.counts[1].item())
        return res


PROBE = _Probe()

# The three switches below exist only so that tests can select the comparison form; nothing else sets
# them (the step A/Bs that are settled are listed in DESIGN.md, "Settled step A/Bs").
# Distinct-row projection in the news towers (False projects every token row: the token-wise form
# the parity tests compare it with; module attributes, not environment switches).
DEDUP_ROWS = True
# Split-K factor of the MHA user encoder's input gradient (dx = dY [Wk; Wv], K = 1152); a split keeps
# >= 512 k per piece.  One-box A/B of the NRMS step, interleaved rounds: unsplit 1.4206-1.4275 ms,
# two pieces 1.4292 ms -- kept unsplit
USER_DGRAD_SPLIT = 1
# CNN word attention (tanh key projection + learned-query pooling) fused per title, forward and
# backward (nr_cnn_keypool_*; False: the key GEMM + pooling kernels the parity tests compare with).
FUSED_KEYPOOL = True


class _TableGradHook:
    """Optional callback ``hook(table_param, dtable) -> bool`` run inside a news-tower backward
    as soon as the dense word-table gradient exists (before the weight-gradient GEMMs).  When it
    returns True it has taken ownership (e.g. started an async all-reduce and will install the
    gradient itself) and the Function returns None for the table."""

    def __init__(self):
        self.fn = None

    def set(self, fn):
        self.fn = fn

    def __call__(self, table, dtable):
        # only a leaf parameter's gradient may be taken over: a non-leaf "table" (an activation,
        # e.g. encoderN(embedding(tokens)) on the unfused path) must flow back through autograd
        if self.fn is None or not _is_param_leaf(table):
            return False
        return bool(self.fn(table, dtable))


def _is_param_leaf(t):
    return t is not None and t.is_leaf and t.requires_grad


TABLE_GRAD_HOOK = _TableGradHook()


def table_grad_buffer(table, V, E, device, zero):
    """The dense [V, E] gradient of a word table.  A table whose rows are sharded across ranks for
    its optimizer step (dist.GradSync(shard_tables=True) sets ``_nr_grad_rows`` = world x slab rows)
    gets a view of a buffer padded to that many rows, so the reduce-scatter runs on the gradient in
    place (no 94 MB copy into a padded send buffer); every other table a plain [V, E] tensor."""
    rows = int(getattr(table, "_nr_grad_rows", 0) or 0) if table is not None else 0
    alloc = torch.zeros if zero else torch.empty
    if rows > V:
        return alloc(rows, E, device=device)[:V]
    return alloc(V, E, device=device)


class _SparseGradHook:
    """Optional callback ``hook(table_param, rows [n] int64, grads [n, E]) -> bool`` for tables whose
    step gradient touches only a few rows (LSTUR's user table: B rows of 876,957).  Returning True
    means the callback owns the gradient (e.g. an exact row-sparse exchange across ranks) and the
    Function returns None for the table instead of a dense [V, E] gradient."""

    def __init__(self):
        self.fn = None

    def set(self, fn):
        self.fn = fn

    def __call__(self, table, rows, grads):
        if self.fn is None or not _is_param_leaf(table):
            return False
        return bool(self.fn(table, rows, grads))


SPARSE_GRAD_HOOK = _SparseGradHook()


class _LocalRowGrad:
    """Single-process gradient of a row-sparse table (LSTUR's user table: B rows of 876,957 per step)
    when no SPARSE_GRAD_HOOK owns it: a dense buffer zeroed ONCE and installed as ``table.grad``; each
    step re-zeroes only the rows the previous step wrote, then scatter-adds this step's rows (instead
    of a 526 MB zero fill per step).  Used only when ``table.grad`` is None at backward time
    (zero_grad(set_to_none=True), as Manager._train and bench do), so gradient accumulation across
    backward passes keeps torch's dense semantics."""

    def __init__(self):
        self.buf, self.prev, self.flags = {}, {}, {}

    def __call__(self, table, rows, grads):
        if not _is_param_leaf(table):
            return False
        if _multi_rank():
            # several ranks and no SPARSE_GRAD_HOOK owning the table (e.g. GradSync(sparse_tables=False)
            # or a DDP-style dense all-reduce): the gradient is reduced densely in place, so other ranks'
            # rows land in it -- this rank's flags and re-zeroing would miss them.  Dense semantics.
            table._nr_row_touched = None
            return False
        key = id(table)
        buf = self.buf.get(key)
        if table.grad is not None:
            # torch's dense accumulation into the existing gradient; if that is our buffer, it now
            # holds rows this class does not track: zero it whole before its next use
            if buf is not None and table.grad.data_ptr() == buf.data_ptr():
                self.prev[key] = None
            table._nr_row_touched = None
            return False
        flags = self.flags.get(key)
        if buf is None or buf.shape != table.shape or buf.device != table.device:
            buf = self.buf[key] = torch.zeros_like(table)
            # per-row "may be non-zero" flags for Adam (it skips reading the rows flagged zero)
            flags = self.flags[key] = torch.zeros(table.shape[0], dtype=torch.uint8, device=table.device)
            self.prev.pop(key, None)
        elif key in self.prev and self.prev[key] is None:
            buf.zero_()
            flags.zero_()
            del self.prev[key]
        prev = self.prev.get(key)
        if prev is not None:
            buf.index_fill_(0, prev, 0.0)
            flags.index_fill_(0, prev, 0)
        # fixed summation order for duplicate ids (no atomics): the same bits every run
        K.rows_add_ordered(grads.reshape(rows.numel(), -1), rows.reshape(-1), buf)
        flags.index_fill_(0, rows.reshape(-1), 1)
        if prev is not None and prev.numel() == rows.numel():
            prev.copy_(rows.reshape(-1))      # in place: a captured step replays the same buffer
        else:
            self.prev[key] = rows.reshape(-1).clone()
        table.grad = buf
        table._nr_row_touched = (buf, flags, buf._version)   # (optim: valid while buf is unmodified)
        return True

    def clear(self):
        self.buf.clear()
        self.prev.clear()
        self.flags.clear()


def _zero_absent_word_rows(table, dtable, ur, pad_row, segsum=None):
    """Zero dtable's rows of ids absent from the batch (and the pad row).  Returns Adam's per-row
    flags (1 = the dgrad stores the row) when the gradient will become ``table.grad`` as it is: a leaf
    table whose ``.grad`` is None (no accumulation into an older gradient) in a single process (a
    dense all-reduce would add other ranks' rows).  None otherwise.  ``segsum`` = (src, dst): the
    multi-token segment sum src -> dst runs with it, the zero fill inside its second launch."""
    track = _is_param_leaf(table) and table.grad is None and not _multi_rank()
    flags = torch.empty(dtable.shape[0], dtype=torch.uint8, device=dtable.device) if track else None
    if segsum is not None:
        return flags if ur.segment_sum_multi_zero(segsum[0], segsum[1], dtable, pad_row, flags) else None
    return flags if ur.zero_absent_rows(dtable, pad_row, flags) else None


def _word_row_flags(table, dtable, flags):
    """Publish (or clear) the word table's row flags for optim.FusedAdam.  The backward only leaves
    them pending, keyed by the gradient buffer's address and version counter; the table's
    post-accumulate-grad hook (_row_flag_hook) turns them into flags bound to the very ``.grad``
    tensor autograd installed (a weak reference to it), and only if that is the buffer, unmodified
    (autograd installs a lone returned gradient as it is; a copy changes the address, an in-place
    accumulation -- another use of the table in the graph, a second backward -- the version).  So the
    flags die with that gradient: after zero_grad(set_to_none) a new gradient the caching allocator
    places at the same address is a different tensor and never picks them up."""
    if _is_param_leaf(table):
        table._nr_row_touched = None
        table._nr_row_pending = ((dtable.data_ptr(), flags, dtable._version)
                                 if dtable is not None and flags is not None else None)
        if getattr(table, "_nr_row_hook", None) is None:
            table._nr_row_hook = table.register_post_accumulate_grad_hook(_row_flag_hook)


def _row_flag_hook(p):
    """Post-accumulate-grad hook of a table with published row flags (see _word_row_flags)."""
    pend = getattr(p, "_nr_row_pending", None)
    p._nr_row_pending = None
    g = p.grad
    if pend is not None and g is not None and g.data_ptr() == pend[0] and g._version == pend[2]:
        p._nr_row_touched = (weakref.ref(g), pend[1], g._version)
    elif isinstance(getattr(p, "_nr_row_touched", None), tuple) and isinstance(p._nr_row_touched[0], weakref.ref):
        p._nr_row_touched = None


def _multi_rank():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


LOCAL_ROW_GRAD = _LocalRowGrad()


class _WgradDeferHook:
    """Optional callback ``hook(run, out) -> bool`` for the news tower's projection weight-gradient
    GEMM (the longest kernel of the backward, issued after the word-table gradient).  ``run(max_cus)``
    launches the GEMM into ``out`` (the zero-filled weight gradient already handed to autograd);
    returning True means the callback launches it later itself -- GradSync's graphed data-parallel
    step runs it in its own graph, beside the word-table all-reduce (twotower.py:49-50's DDP
    overlap of the bucket reduction with the rest of the backward).

    ``max_cus``: CUs the weight-gradient GEMM may occupy while a collective is in flight
    (0 = all), so that RCCL's kernels are not locked out by the GEMM's one-workgroup-per-CU grid."""

    def __init__(self):
        self.fn = None
        self.max_cus = 0

    def set(self, fn, max_cus=0):
        self.fn = fn
        self.max_cus = int(max_cus)

    def __call__(self, run, out):
        if self.fn is None:
            return False
        return bool(self.fn(run, out))


WGRAD_DEFER_HOOK = _WgradDeferHook()


def _word_table_grad(table, dYu, w_b, ur, pad_row, prec, bf16_store, segsum=None, probe=False):
    """The word-table gradient of a distinct-row news tower: dtable[uids] = dYu w_b, one row per
    distinct id of the batch (M = U, not U_pad: no duplicate pad ids), every other row zero.
    dYu [cap, NK]: the per-distinct-row gradient sums; w_b: the weight operand [NK x E]; ``table``:
    the tower's word-table argument (its hooks and row flags hang on it).

    Where the dgrad stores every present row, only the absent rows and the pad row are zero-filled
    instead of the whole table: under bf16x6 (the stream-K tail goes through the workspace, no
    atomics) and, with ``bf16_store``, under bf16 as plain scatter stores (NR_EPI_SCATTER_STORE: no
    atomic tail, which would need zeroed rows).  ``segsum`` = (dY, dYu): the multi-token segment sum
    dY -> dYu is still to run; it runs here, with the zero fill's workgroups in its fix-up launch
    where that fill is the absent-rows one (single process), before it otherwise.  ``probe``: the
    dgrad launch is offered to PROBE as "proj_dgrad".

    -> (dtable, inflight): TABLE_GRAD_HOOK may take the gradient (dtable None, inflight True: the
    table's all-reduce then runs beside the weight gradient that follows)."""
    V, E = table.shape
    absent_only = 0 <= pad_row < V and (prec == L.GEMM_BF16X6 or (bf16_store and prec == L.GEMM_BF16))
    epi = L.EPI_SCATTER_STORE if absent_only and prec == L.GEMM_BF16 else L.EPI_SCATTER_ZEROED
    fold = segsum is not None and absent_only and not _multi_rank()
    if segsum is not None and not fold:
        ur.segment_sum_multi(*segsum)
    dtable = table_grad_buffer(table, V, E, dYu.device, zero=not absent_only)
    rflags = _zero_absent_word_rows(table, dtable, ur, pad_row, segsum if fold else None) if absent_only else None

    def dgrad(dtable=dtable):   # bound now: the hook below may take the name's buffer
        K.gemm_dyn(ur.cap, E, dYu.shape[1], K.operand(dYu, L.KCONTIG), w_b, dtable, m_dev=ur.n_rows,
                   epilogue=epi, c_rows=K.rows_map(ur.uids, L.ROWS_GATHER), pad_row=pad_row, workspace=True)
    if probe:
        PROBE.run("proj_dgrad", dgrad, dtable, ur)
    else:
        dgrad()
    inflight = TABLE_GRAD_HOOK(table, dtable)
    if inflight:
        dtable = None
    _word_row_flags(table, dtable, rflags)
    return dtable, inflight


# ---------------------------------------------------------------------- MHA news encoder

class MHANewsFn(_GradAwareFn):
    """MHA_Encoder.forward (models/Encoders/MHA.py:21-39) on gathered token rows:
    Y = X [Wk; Wv]ᵀ + b  (one GEMM, gather fused)  ->  tied-QK 12-head attention
    -> LayerNorm -> Dropout -> learned-query pooling.   Returns (news [n, H], tok [T, H] or None)."""

    @staticmethod
    def forward(ctx, table, ids, mask, w_cat, b_cat, gamma, beta, query, heads, dk, dv, seq_len,
                pad_row, p_drop, seed, offset, want_tokens, rng=None):
        ctx.prec = K.get_gemm_precision()
        T = ids.numel()
        n = T // seq_len
        V, E = table.shape
        H = heads * dv
        NQ = heads * dk
        NY = NQ + H
        fused = K.mha_pool_supported(seq_len, heads, dk, dv)
        ur = None
        if fused and DEDUP_ROWS:
            # project each distinct word-table row once (Y rows = distinct ids, read through inv);
            # the backward sums dY per distinct row over the unmasked tokens only — the fused
            # tail gives masked tokens an exactly-zero dY (their P rows and columns are zero)
            ur = K.UniqueRows(ids, V, fill_row=pad_row if 0 <= pad_row < V else 0, grad_mask=mask)
            Y = _empty(ur.cap, NY, table)
            PROBE.run("proj_fwd", lambda: K.gemm_dyn(
                ur.cap, NY, E, K.operand(table, L.KCONTIG, rows=ur.uids, mapping=L.ROWS_GATHER),
                K.operand(w_cat, L.KCONTIG), Y, m_dev=ur.u_pad, bias=b_cat), Y, ur)
        else:
            Y = _empty(T, NY, table)
            PROBE.run("proj_fwd", lambda: K.gemm(
                T, NY, E, K.operand(table, L.KCONTIG, rows=ids, mapping=L.ROWS_GATHER),
                K.operand(w_cat, L.KCONTIG), Y, bias=b_cat), Y)
        news = _empty(n, H, table)
        probs = torch.empty(T, device=table.device)
        stats = torch.empty(T, 2, device=table.device)
        tok = _empty(T, H, table) if want_tokens else None
        if fused:
            # attention + LN + dropout + pooling in one kernel per title; when a backward will
            # run, the attention output O is saved too (the split backward reads it instead of recomputing it)
            O = _empty(T, H, table) if _backward_possible(ctx) else None
            # rng (device (seed, offset) snapshot) supersedes the host pair: kernel offset 0
            K.mha_pool_fwd(Y, mask, n, seq_len, heads, dk, dv, gamma, beta, query, news, stats, probs,
                           p_drop=p_drop, seed=seed, offset=0 if rng is not None else offset, zout=tok,
                           yrows=ur.inv if ur else None, rng=rng, oout=O)
        else:
            O = _empty(T, H, table)
            K.mha_attn_fwd(Y[:, :NQ], Y[:, NQ:NY], mask, n, seq_len, heads, dk, dv, O)
            K.attn_pool_fwd(O, query, mask, n, seq_len, news, probs, gamma=gamma, beta=beta, stats=stats,
                            p_drop=p_drop, seed=seed, offset=0 if rng is not None else offset, zout=tok, rng=rng)
        ctx.save_for_backward(table, ids, mask, w_cat, gamma, beta, query, Y, O, probs, stats)
        _reserve_zeros(ctx, table.device, (H,), (H,), (H,), (NY,), (NY, E))
        ctx.cfg = (heads, dk, dv, seq_len, pad_row, p_drop, seed, offset, fused)
        ctx.table_ref = table
        ctx.ur = ur
        ctx.rng = rng
        return news, tok

    @staticmethod
    @_gemm_backward
    def backward(ctx, dnews, dtok):
        table, ids, mask, w_cat, gamma, beta, query, Y, O, probs, stats = ctx.saved_tensors
        _word_row_flags(ctx.table_ref, None, None)
        heads, dk, dv, seq_len, pad_row, p_drop, seed, offset, fused = ctx.cfg
        T = ids.numel()
        n = T // seq_len
        V, E = table.shape
        H = heads * dv
        NQ = heads * dk
        NY = NQ + H
        dnews = dnews.contiguous()
        dq, dgamma, dbeta, db, dw = _backward_zeros(ctx, table.device, (H,), (H,), (H,), (NY,), (NY, E))
        dz = dtok.contiguous() if dtok is not None else None
        ur = ctx.ur
        # one buffer: per-token gradient rows [0, T), then the per-distinct-row sums [T, T + cap); the fused
        # backward writes the row of a token alone in its distinct row's segment straight to the sums
        direct = fused and ur is not None
        dYall = _empty(T + (ur.cap if ur is not None else 0), NY, table)
        dY = dYall[:T]
        # 1. pooling / LayerNorm / attention backward -> dY per token
        if fused:
            # split form: the LN pass's per-token row terms (the head pass rebuilds dO from O with them)
            dob = torch.empty(T, 8, device=table.device) if O is not None else None
            ws = _grad_copies(table.device, 3 * H + NY) if O is not None else None
            K.mha_pool_bwd(Y, mask, n, seq_len, heads, dk, dv, gamma, beta, query, stats, probs, dnews,
                           dYall if direct else dY, db, dq,
                           dgamma, dbeta, p_drop=p_drop, seed=seed, offset=0 if ctx.rng is not None else offset,
                           dz=dz, yrows=ur.inv if ur else None, rng=ctx.rng, o=O, dob=dob, ws=ws,
                           ws_copies=GRAD_COPIES if ws is not None else 0, seg=ur if direct else None, dyu_row0=T)
        else:
            dO = _empty(T, H, table)
            K.attn_pool_bwd(O, query, mask, n, seq_len, probs, dnews, dO, dq, gamma=gamma, beta=beta, stats=stats,
                            dgamma=dgamma, dbeta=dbeta, p_drop=p_drop, seed=seed,
                            offset=0 if ctx.rng is not None else offset, dz=dz, rng=ctx.rng)
            K.mha_attn_bwd(Y[:, :NQ], Y[:, NQ:NY], mask, n, seq_len, heads, dk, dv, dO, dY[:, :NQ], dY[:, NQ:NY],
                           dbias=db)
        dtable = None
        if ur is not None:
            # 2. per-distinct-row sums, then the two GEMMs over U rows instead of T tokens.  After the direct
            # writes only the segments of two or more tokens are left to sum; with a table gradient to come
            # that sum is handed to it (its zero fill can ride in the sum's fix-up launch)
            dYu = dYall[T:]
            if not direct:
                ur.segment_sum(dY, dYu)
            elif not ctx.needs_input_grad[0]:
                ur.segment_sum_multi(dY, dYu)
            # 3. table gradient
            inflight = False
            if ctx.needs_input_grad[0]:
                dtable, inflight = _word_table_grad(ctx.table_ref, dYu, K.operand(w_cat, L.MNCONTIG), ur, pad_row,
                                                    ctx.prec, bf16_store=False,
                                                    segsum=(dY, dYu) if direct else None, probe=True)
            # 4. weight gradient
            prec = ctx.prec

            def wgrad(max_cus=0):
                K.gemm_dyn(NY, E, ur.cap, K.operand(dYu, L.MNCONTIG),
                           K.operand(table, L.MNCONTIG, rows=ur.uids, mapping=L.ROWS_GATHER), dw, k_dev=ur.u_pad,
                           epilogue=L.EPI_ATOMIC, split_k=_split_k(NY, E, ur.cap), prec=prec, max_cus=max_cus,
                           workspace=True)
            if not WGRAD_DEFER_HOOK(wgrad, dw):
                cus = WGRAD_DEFER_HOOK.max_cus if inflight else 0
                PROBE.run("proj_wgrad", lambda: wgrad(cus), dw, ur)
        else:
            if ctx.needs_input_grad[0]:
                dtable = table_grad_buffer(ctx.table_ref, V, E, table.device, zero=True)
                K.gemm(T, E, NY, K.operand(dY, L.KCONTIG), K.operand(w_cat, L.MNCONTIG), dtable,
                       epilogue=L.EPI_SCATTER, c_rows=K.rows_map(ids, L.ROWS_GATHER), pad_row=pad_row)
                if TABLE_GRAD_HOOK(ctx.table_ref, dtable):
                    dtable = None
            _proj_wgrad(dY, K.operand(table, L.MNCONTIG, rows=ids, mapping=L.ROWS_GATHER), dw, None, T)
        return (dtable, None, None, dw, db, dgamma, dbeta, dq.view_as(query), None, None, None, None, None,
                None, None, None, None, None)


# ---------------------------------------------------------------------- CNN news encoder

class CNNNewsFn(torch.autograd.Function):
    """CNN_Encoder.forward (models/Encoders/CNN.py:30-50): Conv1d(E->H, k=3, pad=1) as a
    K = 3E GEMM over CONV3 rows of the table (gather fused) with bias+ReLU epilogue; key =
    tanh(C Wqᵀ + bq) (GEMM, tanh epilogue); learned-query pooling with the token mask.
    ``w3`` is the conv weight as [H][tap*E + e].  Returns (news [n, H], C [T, H])."""

    @staticmethod
    def forward(ctx, table, ids, mask, w3, conv_b, wq, bq, query, seq_len, pad_row):
        # the token output C is rarely consumed: an unused one must not cost a zero-filled gradient
        ctx.set_materialize_grads(False)
        ctx.prec = K.get_gemm_precision()
        T = ids.numel()
        n = T // seq_len
        E = table.shape[1]
        H = w3.shape[0]
        C = _empty(T, H, table)
        K.gemm(T, H, 3 * E, K.operand(table, L.KCONTIG, rows=ids, mapping=L.ROWS_CONV3, seq_len=seq_len, seg=E),
               K.operand(w3, L.KCONTIG), C, bias=conv_b, epilogue=L.EPI_STORE_RELU)
        Kq = _empty(T, H, table)
        K.gemm(T, H, H, K.operand(C, L.KCONTIG), K.operand(wq, L.KCONTIG), Kq, bias=bq, epilogue=L.EPI_STORE_TANH)
        news = _empty(n, H, table)
        probs = torch.empty(T, device=table.device)
        K.attn_pool_fwd(C, query, mask, n, seq_len, news, probs, key=Kq)
        ctx.save_for_backward(table, ids, mask, w3, wq, query, C, Kq, probs)
        ctx.cfg = (seq_len, pad_row)
        ctx.table_ref = table
        return news, C

    @staticmethod
    @_gemm_backward
    def backward(ctx, dnews, dC_out):
        table, ids, mask, w3, wq, query, C, Kq, probs = ctx.saved_tensors
        _word_row_flags(ctx.table_ref, None, None)
        seq_len, pad_row = ctx.cfg
        T = ids.numel()
        n = T // seq_len
        V, E = table.shape
        H = w3.shape[0]
        if dnews is None:   # (grads not materialised) the pooled output unused
            dnews = torch.zeros(n, H, device=table.device)
        dev = table.device
        dnews = dnews.contiguous()
        # dC with its columns padded to a multiple of 32 (zeros): the table dgrad below contracts
        # over H and takes the fast GEMM path only for K % 32 == 0
        Hp = (H + 31) // 32 * 32
        dC_full = torch.zeros(T, Hp, device=dev)
        dC = dC_full[:, :H]
        dKq = _empty(T, H, table)
        dq = torch.zeros(H, device=dev)
        K.attn_pool_bwd(C, query, mask, n, seq_len, probs, dnews, dC, dq, key=Kq, dk=dKq, key_tanh=True,
                        dz=dC_out.contiguous() if dC_out is not None else None)
        # key projection: dWq = dKqᵀ C, dbq = colsum(dKq); dC += dKq Wq, then ReLU'(C)
        dwq, dbq, dconv_b, dw3 = _zeros_views(dev, (H, H), (H,), (H,), (H, 3 * E))
        _proj_wgrad(dKq, K.operand(C, L.MNCONTIG), dwq, dbq, T)
        K.gemm(T, H, H, K.operand(dKq, L.KCONTIG), K.operand(wq, L.MNCONTIG), dC, epilogue=L.EPI_ACCUM_GATE,
               c_rows=K.aux_operand(C))
        _proj_wgrad(dC, K.operand(table, L.MNCONTIG, rows=ids, mapping=L.ROWS_CONV3, seq_len=seq_len, seg=E),
                    dw3, dconv_b, T)
        dtable = None
        if ctx.needs_input_grad[0]:
            dtable = table_grad_buffer(ctx.table_ref, V, E, dev, zero=True)
            w3p = w3 if Hp == H else torch.cat([w3, w3.new_zeros(Hp - H, 3 * E)], 0)
            K.gemm(T, 3 * E, Hp, K.operand(dC_full, L.KCONTIG), K.operand(w3p, L.MNCONTIG), dtable,
                   epilogue=L.EPI_SCATTER, c_rows=K.rows_map(ids, L.ROWS_CONV3, seq_len=seq_len, seg=E),
                   pad_row=pad_row)
            if TABLE_GRAD_HOOK(ctx.table_ref, dtable):
                dtable = None
        return dtable, None, None, dw3, dconv_b, dwq, dbq, dq.view_as(query), None, None


class CNNWeightsFn(torch.autograd.Function):
    """The distinct-row CNN encoder's weight operands (nr_cnn_pack_weights): the Conv1d weight
    [H, E, 3] as w3t [3*Hp, E] (row tap*Hp + h), its transpose w3tt [E, 3*Hp] (the table dgrad's
    K-contiguous weight, 1.5 MB per step) and the key projection zero-padded to [Hp, Hp] / [Hp],
    in one launch; the backward maps the three gradients back in one launch."""

    @staticmethod
    def forward(ctx, conv_w, wq, bq, Hp):
        H, E = conv_w.shape[0], conv_w.shape[1]
        dev = conv_w.device
        w3t = torch.empty(3 * Hp, E, device=dev)
        w3tt = torch.empty(E, 3 * Hp, device=dev)
        wqp = torch.empty(Hp, Hp, device=dev)
        bqp = torch.empty(Hp, device=dev)
        for t in (conv_w, wq, bq):
            if not t.is_contiguous():
                raise L.HipError("cnn weights must be contiguous")
        L.call("nr_cnn_pack_weights", L.ptr(conv_w), L.ptr(wq), L.ptr(bq), H, E, Hp, L.ptr(w3t), L.ptr(wqp),
               L.ptr(bqp), L.ptr(w3tt), L.stream_ptr(conv_w))
        ctx.cfg = (H, E, Hp)
        ctx.mark_non_differentiable(w3tt)
        return w3t, wqp, bqp, w3tt

    @staticmethod
    def backward(ctx, dw3t, dwqp, dbqp, _dw3tt):
        H, E, Hp = ctx.cfg
        dev = (dw3t if dw3t is not None else dwqp).device
        dw3t = dw3t.contiguous() if dw3t is not None else torch.zeros(3 * Hp, E, device=dev)
        dwqp = dwqp.contiguous() if dwqp is not None else torch.zeros(Hp, Hp, device=dev)
        dbqp = dbqp.contiguous() if dbqp is not None else torch.zeros(Hp, device=dev)
        dcw = torch.empty(H, E, 3, device=dev)
        dwq = torch.empty(H, H, device=dev)
        dbq = torch.empty(H, device=dev)
        L.call("nr_cnn_unpack_grads", L.ptr(dw3t), L.ptr(dwqp), L.ptr(dbqp), H, E, Hp, L.ptr(dcw), L.ptr(dwq),
               L.ptr(dbq), L.stream_ptr(dw3t))
        return dcw, dwq, dbq, None


class CNNNewsRowsFn(_GradAwareFn):
    """CNN_Encoder.forward (models/Encoders/CNN.py:30-50) over DISTINCT word rows.

    The k = 3 Conv1d is linear per tap and the embedding lookup (BERT.py:39) is a row gather, so
    they commute: P = table[uids] · [W_0 | W_1 | W_2]ᵀ is ONE GEMM over the U distinct ids of the
    batch (U ≈ 24.6 k of T = 52.8 k tokens on uniform ids), and C[t] = ReLU(b + Σ_j P[inv[t+j-1]][j])
    is a three-row gather-add (nr_conv3_rows_fwd).  The backward sums the shifted dC rows per
    distinct id once (S = nr_segment_rows_sum_conv3), after which the table gradient
    (S · W3 -> plain stores into the distinct rows, no atomics) and the conv weight gradient
    (Sᵀ · table[uids]) are GEMMs over U rows instead of T tokens.

    w3t: [3*Hp, E] with row tap*Hp + h = Conv1d.weight[h, :, tap] (rows h >= H zero); wq, bq: the
    key projection zero-padded to [Hp, Hp] / [Hp] so every contraction has K % 32 == 0; query: the
    pooling query [1, H] (the pooling runs over the padded width, nr_seq_pool_*, with features past
    H of the query and of dnews taken as zero).
    Returns (news [n, H] view, C [T, H] view)."""

    @staticmethod
    def forward(ctx, table, ids, mask, w3t, conv_b, wq, bq, query, seq_len, pad_row, H, w3tt=None):
        # the token output C is rarely consumed: an unused one must not cost a zero-filled gradient
        # (and a padded copy of it) per step
        ctx.set_materialize_grads(False)
        ctx.prec = K.get_gemm_precision()
        T = ids.numel()
        n = T // seq_len
        V, E = table.shape
        Hp = w3t.shape[0] // 3
        ur = K.UniqueRows(ids, V, fill_row=pad_row if 0 <= pad_row < V else 0)
        P = _empty(ur.cap, 3 * Hp, table)
        K.gemm_dyn(ur.cap, 3 * Hp, E, K.operand(table, L.KCONTIG, rows=ur.uids, mapping=L.ROWS_GATHER),
                   K.operand(w3t, L.KCONTIG), P, m_dev=ur.u_pad)
        C = _empty(T, Hp, table)
        K.conv3_rows_fwd(P, Hp, H, ur.inv, seq_len, conv_b, C, relu=True)
        news = _empty(n, Hp, table)
        probs = torch.empty(T, device=table.device)
        fused = FUSED_KEYPOOL and K.cnn_keypool_supported(Hp, seq_len)
        if fused:
            # key projection + tanh + pooling per title; with a backward to come K is kept (the backward
            # reads it instead of recomputing the key products)
            Kq = _empty(T, Hp, table) if _backward_possible(ctx) else None
            K.cnn_keypool_fwd(C, wq, bq, query, mask, n, seq_len, news, probs, qn=H, prec=ctx.prec, kout=Kq)
        else:
            Kq = _empty(T, Hp, table)
            K.gemm(T, Hp, Hp, K.operand(C, L.KCONTIG), K.operand(wq, L.KCONTIG), Kq, bias=bq,
                   epilogue=L.EPI_STORE_TANH)
            # pooling over the padded width: C and Kq are exactly zero past H, and so is the padded query
            K.seq_pool_fwd(C, query, mask, n, seq_len, Hp, news, probs, key=Kq, qn=H)
        ctx.save_for_backward(table, ids, mask, w3t, wq, bq, query, C, Kq, probs, w3tt)
        ctx.cfg = (seq_len, pad_row, H, fused)
        _reserve_zeros(ctx, table.device, (Hp, Hp), (Hp,), (H,), (3 * Hp, E), (H,))
        ctx.table_ref = table
        ctx.ur = ur
        return news[:, :H], C[:, :H]

    @staticmethod
    @_gemm_backward
    def backward(ctx, dnews, dC_out):
        table, ids, mask, w3t, wq, bq, query, C, Kq, probs, w3tt = ctx.saved_tensors
        _word_row_flags(ctx.table_ref, None, None)
        seq_len, pad_row, H, fused = ctx.cfg
        ur = ctx.ur
        T = ids.numel()
        n = T // seq_len
        if dnews is None:   # (grads not materialised) the pooled output unused
            dnews = torch.zeros(n, H, device=table.device)
        V, E = table.shape
        Hp = w3t.shape[0] // 3
        dev = table.device
        dC = _empty(T, Hp, table)
        dwq, dbq, dconv_b, dw3t, dq = _backward_zeros(ctx, dev, (Hp, Hp), (Hp,), (H,), (3 * Hp, E), (H,))
        if dnews.stride(-1) != 1:
            dnews = dnews.contiguous()
        # 1. pooling / key projection backward -> dC per token
        if fused:
            # one pass per title: K read back (or recomputed without it), pooling / tanh / key-projection
            # backward, ReLU gate, dWq / dbq / dq / dconv_b summed over per-workgroup partials
            dz = dC_out if dC_out is None or dC_out.stride(-1) == 1 else dC_out.contiguous()
            K.cnn_keypool_bwd(C, wq, bq, query, n, seq_len, H, probs, dnews, dC, dwq, dbq, dq, dconv_b, dz=dz,
                              prec=ctx.prec, kin=Kq)
        else:
            dKq = _empty(T, Hp, table)
            # dC = p dnews (+ dC_out), dKq = ds q (1 - Kq²) over the padded width: exactly zero past H
            # (dnews and the query count as zero there)
            dz = torch.nn.functional.pad(dC_out, (0, Hp - H)) if dC_out is not None else None
            K.seq_pool_bwd(C, query, mask, n, seq_len, Hp, probs, dnews, dC, dq, key=Kq, dk=dKq, key_tanh=True,
                           dz=dz, qn=H)
            # key projection: dWq = dKqᵀ C, dbq = colsum(dKq); dC = ReLU'(C) ⊙ (dC + dKq Wq) (padded
            # columns of C are zero, so the gate also zeroes dC's padding)
            _proj_wgrad(dKq, K.operand(C, L.MNCONTIG), dwq, dbq, T)
            K.gemm(T, Hp, Hp, K.operand(dKq, L.KCONTIG), K.operand(wq, L.MNCONTIG), dC, epilogue=L.EPI_ACCUM_GATE,
                   c_rows=K.aux_operand(C))
            K.colsum(dC, T, H, dconv_b)
        # 2. per-distinct-row sums of the shifted dC rows
        S = _empty(ur.cap, 3 * Hp, table)
        ur.segment_sum_conv3(dC, S, Hp, seq_len)
        # 3. table gradient, over the weights transposed by the pack launch so both operands are k-contiguous
        dtable = None
        inflight = False
        if ctx.needs_input_grad[0]:
            w_b = K.operand(w3tt if w3tt is not None else w3t.t().contiguous(), L.KCONTIG)
            dtable, inflight = _word_table_grad(ctx.table_ref, S, w_b, ur, pad_row, ctx.prec, bf16_store=True)
        # 4. weight gradient (split-K partials through the workspace under bf16 and bf16x6)
        K.gemm_dyn(3 * Hp, E, ur.cap, K.operand(S, L.MNCONTIG),
                   K.operand(table, L.MNCONTIG, rows=ur.uids, mapping=L.ROWS_GATHER), dw3t, k_dev=ur.u_pad,
                   epilogue=L.EPI_ATOMIC, split_k=_split_k(3 * Hp, E, ur.cap),
                   max_cus=WGRAD_DEFER_HOOK.max_cus if inflight else 0,
                   workspace=ctx.prec in (L.GEMM_BF16, L.GEMM_BF16X6))
        return (dtable, None, None, dw3t, dconv_b, dwq, dbq, dq.view_as(query), None, None, None, None)


# ---------------------------------------------------------------------- pooling user encoder

class AttnPoolFn(_GradAwareFn):
    """Attention_Pooling.forward (models/Encoders/Pooling.py:12-25): learned-query pooling of
    the history with the history mask.  x: [B*N, H] rows view; returns [B, H]."""

    @staticmethod
    def forward(ctx, x, query, mask, B, N):
        H = query.numel()
        probs = torch.empty(B * N, device=x.device)
        # one wave per sequence (nr_seq_pool_*) when the rows are float4-addressable
        sp = K.seq_pool_supported(H, N) and x.stride(-1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
        out = _empty(B, H, x)
        if sp:
            K.seq_pool_fwd(x, query, mask, B, N, H, out, probs)
        else:
            K.attn_pool_fwd(x, query, mask, B, N, out, probs)
        ctx.save_for_backward(x, query, mask, probs)
        ctx.cfg = (B, N, H, sp)
        ctx.dx_dest = GRAD_DEST.take(x)
        _reserve_zeros(ctx, x.device, (H,))
        return out

    @staticmethod
    def backward(ctx, dout):
        x, query, mask, probs = ctx.saved_tensors
        B, N, H, sp = ctx.cfg
        dx = _grad_out(ctx.dx_dest, B * N, H, x)
        dq, = _backward_zeros(ctx, x.device, (H,))
        if sp:
            K.seq_pool_bwd(x, query, mask, B, N, H, probs, dout if dout.stride(-1) == 1 else dout.contiguous(), dx, dq)
            return dx, dq.view_as(query), None, None, None
        K.attn_pool_bwd(x, query, mask, B, N, probs, dout.contiguous(), dx, dq)
        return dx, dq.view_as(query), None, None, None


# ---------------------------------------------------------------------- MHA over rows

class MHAFn(_GradAwareFn):
    """MultiheadAttention.forward (models/Modules/Attention.py:115-147) on plain rows:
    Y = x [Wk; Wv]ᵀ + b (GEMM) -> tied-QK attention core (pairwise token mask).
    x: [nseq*L, D] -> [nseq*L, heads*dv].  Used by MHA_User_Encoder (MHA.py:58-75) and the
    standalone MultiheadAttention module."""

    @staticmethod
    def forward(ctx, x, mask, w_cat, b_cat, nseq, seq_len, heads, dk, dv):
        ctx.prec = K.get_gemm_precision()
        D = x.shape[1]
        NQ = heads * dk
        NY = w_cat.shape[0]
        rows = nseq * seq_len
        Y = _empty(rows, NY, x)
        K.gemm(rows, NY, D, K.operand(x, L.KCONTIG), K.operand(w_cat, L.KCONTIG), Y, bias=b_cat)
        O = _empty(rows, heads * dv, x)
        K.mha_attn_fwd(Y[:, :NQ], Y[:, NQ:NY], mask, nseq, seq_len, heads, dk, dv, O)
        ctx.save_for_backward(x, mask, w_cat, Y)
        ctx.cfg = (nseq, seq_len, heads, dk, dv)
        ctx.dx_dest = GRAD_DEST.take(x)
        _reserve_zeros(ctx, x.device, (NY, D), (NY,))
        return O

    @staticmethod
    @_gemm_backward
    def backward(ctx, dO):
        x, mask, w_cat, Y = ctx.saved_tensors
        nseq, seq_len, heads, dk, dv = ctx.cfg
        D = x.shape[1]
        NQ = heads * dk
        NY = w_cat.shape[0]
        rows = nseq * seq_len
        dev = x.device
        if dO.stride(-1) != 1 or dO.stride(0) % 4 or dO.data_ptr() % 16:
            dO = dO.contiguous()
        dY = _empty(rows, NY, x)
        dw, db = _backward_zeros(ctx, dev, (NY, D), (NY,))
        # the projection bias gradient (column sums of dY) accumulates inside the attention backward
        K.mha_attn_bwd(Y[:, :NQ], Y[:, NQ:NY], mask, nseq, seq_len, heads, dk, dv, dO, dY[:, :NQ], dY[:, NQ:NY],
                       dbias=db)
        split = USER_DGRAD_SPLIT if NY >= 512 * USER_DGRAD_SPLIT else 1
        if split > 1:
            # few output tiles (1600 x 384 for the NRMS user encoder) over a long contraction (1152): split
            # K and add the pieces atomically into a zeroed dx
            dx = torch.zeros(rows, D, device=dev)
            K.gemm(rows, D, NY, K.operand(dY, L.KCONTIG), K.operand(w_cat, L.MNCONTIG), dx, epilogue=L.EPI_ATOMIC,
                   split_k=split)
            _proj_wgrad(dY, K.operand(x, L.MNCONTIG), dw, None, rows)
        else:
            # dx = dY W and dW += dYᵀ x read the same dY and depend on nothing else: one launch
            # (_proj_wgrad's GEMM without a bias gradient: db came from the attention backward)
            dx = _grad_out(ctx.dx_dest, rows, D, x)
            K.gemm_pair(K.gemm_desc(rows, D, NY, K.operand(dY, L.KCONTIG), K.operand(w_cat, L.MNCONTIG), dx),
                        K.gemm_desc(NY, D, rows, K.operand(dY, L.MNCONTIG), K.operand(x, L.MNCONTIG), dw,
                                    epilogue=L.EPI_ATOMIC, split_k=_split_k(NY, D, rows)), dx)
        return dx, None, dw, db, None, None, None, None, None


# ---------------------------------------------------------------------- recurrent user encoders

class RNNUserFn(_GradAwareFn):
    """RNN_User_Encoder (RNN.py:50-73) and LSTUR_User_Encoder (RNN.py:88-104):
    gx = x W_ihᵀ + b_ih for all steps (GEMM) -> sequential cell kernel -> h at step len-1.
    LSTUR: reverse=True, mask=None (all N steps), h0 = user_table[h0_idx]."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, user_table, cell, mask, B, N, reverse, h0_idx):
        ctx.prec = K.get_gemm_precision()
        H = x.shape[1]
        G = 4 if cell == L.CELL_LSTM else 3
        dev = x.device
        ctx.dx_dest = GRAD_DEST.take(x)   # (before x is padded below)
        gx = _empty(B * N, G * H, x)
        # the input projection contracts over H: padded to a multiple of 32 with zero columns (a 1 MB
        # copy of x, 0.4 MB of w_ih) it runs on the fast GEMM path instead of the generic one
        Hp = _ceil32(H)
        if Hp != H:
            x = torch.nn.functional.pad(x, (0, Hp - H))
            w_k = torch.nn.functional.pad(w_ih.detach(), (0, Hp - H))
        else:
            w_k = w_ih
        K.gemm(B * N, G * H, Hp, K.operand(x, L.KCONTIG), K.operand(w_k, L.KCONTIG), gx, bias=b_ih)
        gates = torch.empty(B * N, 4 * H, device=dev)
        hprev = torch.empty(B * N, H, device=dev)
        cprev = torch.empty(B * N, H, device=dev) if cell == L.CELL_LSTM else None
        hout = _empty(B, H, x)
        whh_t = w_hh.detach().t().contiguous()
        K.rnn_fwd(cell, gx, whh_t, b_hh, B, N, H, gates, hprev, cprev, hout,
                  h0=user_table if user_table is not None else None, h0_idx=h0_idx, mask=mask, reverse=reverse)
        ctx.save_for_backward(x, w_ih, w_hh, gates, hprev, cprev, mask, h0_idx, user_table)
        ctx.cfg = (cell, B, N, reverse)
        _reserve_zeros(ctx, dev, (G * H, H), (G * H,), (G * H, H), (G * H,))
        ctx.table_ref = user_table
        return hout

    @staticmethod
    @_gemm_backward
    def backward(ctx, dh):
        x, w_ih, w_hh, gates, hprev, cprev, mask, h0_idx, user_table = ctx.saved_tensors
        cell, B, N, reverse = ctx.cfg
        H = w_ih.shape[1]
        Hp = x.shape[1]            # x saved zero-padded to a multiple of 32 columns (forward)
        G = 4 if cell == L.CELL_LSTM else 3
        GH = G * H
        GHp = _ceil32(GH) if Hp != H else GH
        dev = x.device
        # the gate gradients with zero columns up to GHp (the dx GEMM contracts over them) and the
        # padded operands below keep the three GEMMs on the fast path (K % 32 == 0, float4 rows)
        dgi_b = torch.empty(B * N, GHp, device=dev)
        dgh_b = torch.empty(B * N, GHp, device=dev) if cell == L.CELL_GRU else None
        for t in (dgi_b, dgh_b):
            if t is not None and GHp != GH:
                t[:, GH:].zero_()
        dgi = dgi_b[:, :GH]
        dgh = dgh_b[:, :GH] if dgh_b is not None else None
        dh0 = torch.empty(B, H, device=dev) if user_table is not None else None
        K.rnn_bwd(cell, w_hh.contiguous(), gates, hprev, cprev, B, N, H, dh.contiguous(), dgi, dgh=dgh, dh0=dh0,
                  mask=mask, reverse=reverse)
        dgh_ = dgi if dgh is None else dgh
        dx = _grad_out(ctx.dx_dest, B * N, H, x)
        if Hp != H:
            w_k = torch.nn.functional.pad(w_ih.detach(), (0, Hp - H, 0, GHp - GH))
            K.gemm(B * N, H, GHp, K.operand(dgi_b, L.KCONTIG), K.operand(w_k, L.MNCONTIG), dx)
            h_k = torch.nn.functional.pad(hprev, (0, Hp - H))
        else:
            K.gemm(B * N, H, GH, K.operand(dgi, L.KCONTIG), K.operand(w_ih, L.MNCONTIG), dx)
            h_k = hprev
        dw_ih, db_ih, dw_hh, db_hh = _backward_zeros(ctx, dev, (GH, H), (GH,), (GH, H), (GH,))
        _proj_wgrad(dgi, K.operand(x, L.MNCONTIG), dw_ih, db_ih, B * N)
        _proj_wgrad(dgh_, K.operand(h_k, L.MNCONTIG), dw_hh, db_hh, B * N)
        dtab = None
        if user_table is not None and ctx.needs_input_grad[5]:
            if not SPARSE_GRAD_HOOK(ctx.table_ref, h0_idx, dh0) and not LOCAL_ROW_GRAD(ctx.table_ref, h0_idx, dh0):
                dtab = torch.zeros_like(user_table)
                K.embedding_bwd(dh0, h0_idx, dtab, padding_idx=None)
        return dx, dw_ih, dw_hh, db_ih, db_hh, dtab, None, None, None, None, None, None


# ---------------------------------------------------------------------- bidirectional-LSTM news encoder

class RNNNewsFn(_GradAwareFn):
    """RNN_Encoder.forward (models/Encoders/RNN.py:17-33) on gathered token rows: the input projections
    of both directions are ONE GEMM [T, 8H, E] (gather fused, b_ih in the epilogue), then the batched
    recurrence nr_birnn_fwd.  All L steps run, padding tokens are ordinary inputs (there is no mask).
    Returns (news [n, H], tok [T, H] or None)."""

    @staticmethod
    def forward(ctx, table, ids, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r, seq_len, pad_row,
                want_tokens):
        # an unused token output must not cost a zero-filled gradient
        ctx.set_materialize_grads(False)
        ctx.prec = K.get_gemm_precision()
        T = ids.numel()
        n = T // seq_len
        H = w_hh.shape[1]
        GH = 8 * H
        dev = table.device
        w_cat = torch.cat([w_ih.detach(), w_ih_r.detach()], 0)            # [8H, E]
        b_cat = torch.cat([b_ih.detach(), b_ih_r.detach()], 0)
        bhh = torch.stack([b_hh.detach(), b_hh_r.detach()])
        gx = _empty(T, GH, table)
        K.gemm(T, GH, table.shape[1], K.operand(table, L.KCONTIG, rows=ids, mapping=L.ROWS_GATHER),
               K.operand(w_cat, L.KCONTIG), gx, bias=b_cat)
        whh_f, whh_b = K.birnn_pack_whh(w_hh, w_hh_r)
        gates = torch.empty(K.birnn_gates_numel(n, seq_len, H), device=dev)
        # h_{t-1} of both directions, rows padded with zero columns to a multiple of 32 (the dW_hh operand)
        Hp = _ceil32(H)
        hprev = torch.empty(2, T, Hp, device=dev)
        if Hp != H:
            hprev[:, :, H:].zero_()
        hlast = torch.empty(2, n, H, device=dev)
        news = _empty(n, H, table)
        tok = _empty(T, H, table) if want_tokens else None
        K.birnn_fwd(gx, whh_f, bhh, n, seq_len, H, gates, hprev, hlast, news, tok=tok)
        ctx.save_for_backward(table, ids, w_cat, whh_b, gates, hprev)
        ctx.cfg = (seq_len, pad_row, H)
        ctx.table_ref = table
        return news, tok

    @staticmethod
    @_gemm_backward
    def backward(ctx, dnews, dtok):
        table, ids, w_cat, whh_b, gates, hprev = ctx.saved_tensors
        _word_row_flags(ctx.table_ref, None, None)
        seq_len, pad_row, H = ctx.cfg
        T = ids.numel()
        n = T // seq_len
        V, E = table.shape
        GH = 8 * H
        dev = table.device
        if dnews is None and dtok is None:
            return (None,) * 13
        # the gate gradients with zero columns up to a multiple of 32: the table dgrad contracts over them
        GHp = _ceil32(GH)
        dg_full = torch.empty(T, GHp, device=dev)
        if GHp != GH:
            dg_full[:, GH:].zero_()
        dg = dg_full[:, :GH]
        K.birnn_bwd(whh_b, gates, n, seq_len, H, dg, dnews=dnews.contiguous() if dnews is not None else None,
                    dtok=dtok.contiguous() if dtok is not None else None)
        dw_cat, db_cat, dw_hh, dw_hh_r = _zeros_views(dev, (GH, E), (GH,), (4 * H, H), (4 * H, H))
        _proj_wgrad(dg, K.operand(table, L.MNCONTIG, rows=ids, mapping=L.ROWS_GATHER), dw_cat, db_cat, T)
        _proj_wgrad(dg[:, :4 * H], K.operand(hprev[0], L.MNCONTIG), dw_hh, None, T)
        _proj_wgrad(dg[:, 4 * H:], K.operand(hprev[1], L.MNCONTIG), dw_hh_r, None, T)
        dtable = None
        if ctx.needs_input_grad[0]:
            dtable = table_grad_buffer(ctx.table_ref, V, E, dev, zero=True)
            w_p = w_cat if GHp == GH else torch.cat([w_cat, w_cat.new_zeros(GHp - GH, E)], 0)
            K.gemm(T, E, GHp, K.operand(dg_full, L.KCONTIG), K.operand(w_p, L.MNCONTIG), dtable,
                   epilogue=L.EPI_SCATTER, c_rows=K.rows_map(ids, L.ROWS_GATHER), pad_row=pad_row)
            if TABLE_GRAD_HOOK(ctx.table_ref, dtable):
                dtable = None
        db_hh = db_cat.clone()   # the recurrent bias enters the same pre-activations as b_ih
        return (dtable, None, dw_cat[:4 * H], dw_hh, db_cat[:4 * H], db_hh[:4 * H], dw_cat[4 * H:], dw_hh_r,
                db_cat[4 * H:], db_hh[4 * H:], None, None, None)


# ---------------------------------------------------------------------- one-layer BERT news encoder

BERT_LN_EPS = 1e-12   # BertConfig().layer_norm_eps


class TransformerNewsFn(_GradAwareFn):
    """Transformer_Encoder.forward (models/Encoders/Transformer.py, models/Modules/OneLayerBert.py) on
    gathered token rows: the [T, H, E] projection (gather fused), ONE [T, 3H, H] GEMM for query / key /
    value, the one-head attention core nr_sha_attn_fwd (XSoftmax with the key mask, dropout on the
    probabilities; always f32), dense + add + LayerNorm, the [T, 4H, H] GEMM with the GELU epilogue,
    the [T, H, 4H] GEMM + add + LayerNorm, and the learned-query pooling over the tokens themselves
    (nr_seq_pool_fwd without a key).  ``params``: project w, b; query / key / value w, b;
    attention.output dense w, b, LayerNorm w, b; intermediate dense w, b; output dense w, b,
    LayerNorm w, b; query_words.  ``drop``: (p_attn, p_attn_out, p_out, seed, offset) with ``rng`` the
    device snapshot of one counter range of T*L + 2*T*H (sites in that order), or None (eval).
    Returns (news [n, H], tok [T, H] or None)."""

    @staticmethod
    def forward(ctx, table, ids, mask, seq_len, pad_row, want_tokens, drop, rng, *params):
        # an unused token output must not cost a zero-filled gradient
        ctx.set_materialize_grads(False)
        ctx.prec = K.get_gemm_precision()
        wp, bp, wq, bq, wk, bk, wv, bv, wo, bo, l1w, l1b, wi, bi, wo2, bo2, l2w, l2b, query = \
            [p.detach() for p in params]
        T = ids.numel()
        n = T // seq_len
        E = table.shape[1]
        H = wp.shape[0]
        dev = table.device

        def site(k):
            """The kernels' dropout arguments of site k (0 attention, 1 attention output, 2 output)."""
            if drop is None or drop[k] <= 0.0:
                return dict(p_drop=0.0)
            rel = (0, T * seq_len, T * seq_len + T * H)[k]
            if rng is not None:    # the kernels add rel to the snapshot's device offset
                return dict(p_drop=drop[k], seed=drop[3], offset=rel, rng=rng)
            return dict(p_drop=drop[k], seed=drop[3], offset=drop[4] + rel)

        x0 = _empty(T, H, table)
        K.gemm(T, H, E, K.operand(table, L.KCONTIG, rows=ids, mapping=L.ROWS_GATHER), K.operand(wp, L.KCONTIG), x0,
               bias=bp)
        wqkv = torch.cat([wq, wk, wv], 0)
        qkv = _empty(T, 3 * H, table)
        K.gemm(T, 3 * H, H, K.operand(x0, L.KCONTIG), K.operand(wqkv, L.KCONTIG), qkv, bias=torch.cat([bq, bk, bv], 0))
        cx = _empty(T, H, table)
        probs = torch.empty(T * seq_len, device=dev)
        K.sha_attn_fwd(qkv, mask, n, seq_len, H, cx, probs, **site(0))
        a = _empty(T, H, table)
        K.gemm(T, H, H, K.operand(cx, L.KCONTIG), K.operand(wo, L.KCONTIG), a, bias=bo)
        h1 = _empty(T, H, table)
        st1 = torch.empty(T, 2, device=dev)
        K.bert_add_ln_fwd(a, x0, l1w, l1b, BERT_LN_EPS, h1, st1, **site(1))
        U = _empty(T, 4 * H, table)
        G = _empty(T, 4 * H, table)
        K.gemm(T, 4 * H, H, K.operand(h1, L.KCONTIG), K.operand(wi, L.KCONTIG), G, bias=bi,
               epilogue=L.EPI_STORE_GELU, c_rows=K.operand(U, L.KCONTIG))
        o = _empty(T, H, table)
        K.gemm(T, H, 4 * H, K.operand(G, L.KCONTIG), K.operand(wo2, L.KCONTIG), o, bias=bo2)
        h2 = _empty(T, H, table)
        st2 = torch.empty(T, 2, device=dev)
        K.bert_add_ln_fwd(o, h1, l2w, l2b, BERT_LN_EPS, h2, st2, **site(2))
        news = _empty(n, H, table)
        pprobs = torch.empty(T, device=dev)
        K.seq_pool_fwd(h2, query, mask, n, seq_len, H, news, pprobs)
        ctx.save_for_backward(table, ids, mask, wp, wqkv, wo, l1w, wi, wo2, l2w, query, x0, qkv, cx, probs, a, st1,
                              h1, U, G, o, st2, h2, pprobs)
        ctx.cfg = (seq_len, pad_row, H)
        ctx.site = site
        ctx.table_ref = table
        return news, (h2 if want_tokens else None)

    @staticmethod
    @_gemm_backward
    def backward(ctx, dnews, dtok):
        (table, ids, mask, wp, wqkv, wo, l1w, wi, wo2, l2w, query, x0, qkv, cx, probs, a, st1, h1, U, G, o, st2, h2,
         pprobs) = ctx.saved_tensors
        _word_row_flags(ctx.table_ref, None, None)
        seq_len, pad_row, H = ctx.cfg
        site = ctx.site
        T = ids.numel()
        n = T // seq_len
        V, E = table.shape
        dev = table.device
        if dnews is None and dtok is None:
            return (None,) * 27
        if dnews is None:
            dnews = torch.zeros(n, H, device=dev)
        elif dnews.stride(-1) != 1:
            dnews = dnews.contiguous()
        if dtok is not None and (dtok.stride(-1) != 1 or dtok.stride(0) % 4 or dtok.data_ptr() % 16):
            dtok = dtok.contiguous()
        (dwp, dbp, dwqkv, dbqkv, dwo, dbo, dl1w, dl1b, dwi, dbi, dwo2, dbo2, dl2w, dl2b, dq) = _zeros_views(
            dev, (H, E), (H,), (3 * H, H), (3 * H,), (H, H), (H,), (H,), (H,), (4 * H, H), (4 * H,), (H, 4 * H), (H,),
            (H,), (H,), (H,))
        # pooling: dh2 = p dnews + ds q (+ dtok)
        dh2 = _empty(T, H, table)
        K.seq_pool_bwd(h2, query, mask, n, seq_len, H, pprobs, dnews, dh2, dq, dz=dtok)
        # BertOutput, BertIntermediate
        dh1 = _empty(T, H, table)
        do = _empty(T, H, table)
        K.bert_add_ln_bwd(o, h1, l2w, st2, dh2, dh1, do, dl2w, dl2b, **site(2))
        dU = _empty(T, 4 * H, table)
        K.gemm(T, 4 * H, H, K.operand(do, L.KCONTIG), K.operand(wo2, L.MNCONTIG), dU, epilogue=L.EPI_GELU_GRAD,
               c_rows=K.operand(U, L.KCONTIG))
        _proj_wgrad(do, K.operand(G, L.MNCONTIG), dwo2, dbo2, T)
        K.gemm(T, H, 4 * H, K.operand(dU, L.KCONTIG), K.operand(wi, L.MNCONTIG), dh1, epilogue=L.EPI_ACCUM)
        _proj_wgrad(dU, K.operand(h1, L.MNCONTIG), dwi, dbi, T)
        # BertSelfOutput, the attention core, query / key / value
        dx0 = _empty(T, H, table)
        da = _empty(T, H, table)
        K.bert_add_ln_bwd(a, x0, l1w, st1, dh1, dx0, da, dl1w, dl1b, **site(1))
        dcx = _empty(T, H, table)
        K.gemm(T, H, H, K.operand(da, L.KCONTIG), K.operand(wo, L.MNCONTIG), dcx)
        _proj_wgrad(da, K.operand(cx, L.MNCONTIG), dwo, dbo, T)
        dqkv = _empty(T, 3 * H, table)
        K.sha_attn_bwd(qkv, mask, n, seq_len, H, probs, dcx, dqkv, **site(0))
        K.gemm(T, H, 3 * H, K.operand(dqkv, L.KCONTIG), K.operand(wqkv, L.MNCONTIG), dx0, epilogue=L.EPI_ACCUM)
        _proj_wgrad(dqkv, K.operand(x0, L.MNCONTIG), dwqkv, dbqkv, T)
        # the projection and the word table
        _proj_wgrad(dx0, K.operand(table, L.MNCONTIG, rows=ids, mapping=L.ROWS_GATHER), dwp, dbp, T)
        dtable = None
        if ctx.needs_input_grad[0]:
            dtable = table_grad_buffer(ctx.table_ref, V, E, dev, zero=True)
            K.gemm(T, E, H, K.operand(dx0, L.KCONTIG), K.operand(wp, L.MNCONTIG), dtable, epilogue=L.EPI_SCATTER,
                   c_rows=K.rows_map(ids, L.ROWS_GATHER), pad_row=pad_row)
            if TABLE_GRAD_HOOK(ctx.table_ref, dtable):
                dtable = None
        return (dtable, None, None, None, None, None, None, None, dwp, dbp, dwqkv[:H], dbqkv[:H], dwqkv[H:2 * H],
                dbqkv[H:2 * H], dwqkv[2 * H:], dbqkv[2 * H:], dwo, dbo, dl1w, dl1b, dwi, dbi, dwo2, dbo2, dl2w, dl2b,
                dq.view_as(query))


# ---------------------------------------------------------------------- scorer

class ScoreFn(torch.autograd.Function):
    """compute_score + log_softmax (training) / sigmoid (eval)
    (models/TwoTowerBaseModel.py:51-75).  cdd [B*C, H] rows view, user [B, H] -> [B, C]."""

    @staticmethod
    def forward(ctx, cdd, user, B, C, mode):
        H = user.shape[1]
        logits = torch.empty(B, C, device=user.device)
        K.score_fwd(cdd, user, B, C, H, mode, logits)
        ctx.save_for_backward(cdd, user, logits)
        ctx.cfg = (B, C, mode)
        ctx.dcdd_dest = GRAD_DEST.take(cdd)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        cdd, user, logits = ctx.saved_tensors
        B, C, mode = ctx.cfg
        H = user.shape[1]
        dcdd = _grad_out(ctx.dcdd_dest, B * C, H, user)
        duser = _empty(B, H, user)
        K.score_bwd(cdd, user, logits, dlogits.contiguous(), B, C, H, mode, dcdd, duser)
        return dcdd, duser, None, None, None


class ScoreNLLFn(torch.autograd.Function):
    """compute_score + log_softmax (models/TwoTowerBaseModel.py:51-75) and Manager._train's
    NLLLoss (utils/Manager.py:382,641; reduction 'mean') in one kernel each way.
    -> (logits [B, C], loss []); the backward takes either gradient or both."""

    @staticmethod
    def forward(ctx, cdd, user, B, C, label):
        H = user.shape[1]
        logits = torch.empty(B, C, device=user.device)
        loss = torch.empty((), device=user.device)
        label = label.to(user.device).reshape(-1)
        label = label if label.is_contiguous() else label.contiguous()
        K.score_nll_fwd(cdd, user, label, B, C, H, logits, loss)
        ctx.save_for_backward(cdd, user, logits, label)
        ctx.cfg = (B, C)
        ctx.dcdd_dest = GRAD_DEST.take(cdd)
        ctx.set_materialize_grads(False)
        return logits, loss

    @staticmethod
    def backward(ctx, dlogits, dloss):
        cdd, user, logits, label = ctx.saved_tensors
        B, C = ctx.cfg
        H = user.shape[1]
        dcdd = _grad_out(ctx.dcdd_dest, B * C, H, user)
        duser = _empty(B, H, user)
        if dlogits is not None and not dlogits.is_contiguous():
            dlogits = dlogits.contiguous()
        K.score_nll_bwd(cdd, user, logits, label, dloss, dlogits, B, C, H, dcdd, duser)
        return dcdd, duser, None, None, None


class EmbeddingFn(torch.autograd.Function):
    """BERT_Embedding.forward (models/Embeddings/BERT.py:24-40): row gather; the backward is
    a padding_idx-aware scatter-add into a dense table gradient (embedding_dense_backward)."""

    @staticmethod
    def forward(ctx, table, ids, padding_idx):
        out = torch.empty(ids.numel(), table.shape[1], device=table.device)
        K.embedding_fwd(table, ids, out)
        ctx.save_for_backward(ids)
        ctx.cfg = (tuple(table.shape), padding_idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        shape, pad = ctx.cfg
        dtable = torch.zeros(shape, device=dout.device)
        K.embedding_bwd(dout.contiguous(), ids, dtable, padding_idx=pad)
        return dtable, None, None
