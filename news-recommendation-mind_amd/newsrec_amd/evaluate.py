"""Fast evaluation pipeline: Manager._eval_fast (utils/Manager.py:474-541),
Manager.evaluate (:544-590) and cal_metric (:1205-1345), MI355X-first.

The reference encodes the news table on rank 0 only, saves it with torch.save, barriers, reloads
it on every rank, then scores one impression at a time (loader batch size 1) and gathers Python
lists with all_gather_object.  Here:

  encode_news_table   every rank encodes a contiguous shard of the news rows (fused gather +
                      encoder kernels, eval mode) and one RCCL all_gather_into_tensor assembles
                      the [N+1, H] table on every GPU -- no disk round trip
  predict_fast_batch  a batch of impression chunks at once: the user tower over the chunks'
                      histories, then ONE ragged scorer launch over all their candidates
                      (nr_score_ragged: table row . user row / sqrt(H), sigmoid)
  eval_fast           the rank's Partition_Sampler chunk range, then one padded RCCL all-gather
                      of the predictions to rank 0 (instead of all_gather_object of lists)
  cal_metric          per-impression AUC / MRR / nDCG@k / hit@k in one HIP launch
                      (nr_impression_metrics), then the reference's np.mean + round(4)
  test                Manager.test (:815-852) minus checkpoint loading: eval_fast on a test split,
                      then prediction.txt with the per-impression ordinal ranks and the text of
                      every line formed on the device (nr_rank_ordinal, nr_format_prediction)
                      and copied to the file in bounded slabs
  topk_news / recommend / recall_metrics   dense recall (--mode recall -rt d): the K best rows of the
                      whole encoded table per user (nr_topk_news) and recall@k / hit@k
  build_bm25_index / sparse_topk_news / merge_recall   sparse recall (-rt s, sd): the reference's
                      token-level BM25 inverted index (utils.py:219-246, :287-342) built on the device
                      and the exact top-K search over it (nr_bm25_*); recommend(recall_type=...)

history_from_table: the reference re-encodes each impression's history titles inside
predict_fast (TwoTowerBaseModel.py:78-83 calls encode_user).  In eval mode the encoder is
deterministic and row-independent, so the history representations equal the news table's rows
for the same news ids; reading them from the table is the same result without re-running the
news tower (test_mind_gpu.py checks the two paths agree).
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L
from . import kernels as K


def _chunk_range(n_chunks, world, rank):
    """Partition_Sampler (utils.py:267-283): contiguous chunks, the last rank takes the rest."""
    per, extra = divmod(n_chunks, world)
    lo = per * rank
    return lo, lo + per + (extra if rank + 1 == world else 0)


def _world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


@torch.no_grad()
def encode_news_table(model, store, batch_news=8192, group=None):
    """Manager._eval_fast step 1 (Manager.py:490-509): news_reprs[cdd_id] = encode_news(x) for every
    row of the split's news table (row 0 included, as MIND_news yields it, MIND.py:471-491),
    sharded over the ranks of ``group`` and all-gathered.  -> [N+1, H] fp32 on every rank."""
    world, rank = _world(group)
    was_training = model.training
    model.eval()
    model.init_encoding()
    N = store.n_news
    H = model.hidden_dim
    per = -(-N // world)
    lo, hi = rank * per, min((rank + 1) * per, N)
    shard = torch.zeros(per, H, dtype=torch.float32, device=store.device)
    for s in range(lo, hi, batch_news):
        e = min(s + batch_news, hi)
        x = {"cdd_encoded_index": store.tok[s:e].to(torch.int64).unsqueeze(1),
             "cdd_attn_mask": store.attn[s:e].to(torch.int64).unsqueeze(1)}
        shard[s - lo:e - lo] = model.encode_news(x).squeeze(-2)
    model.destroy_encoding()
    model.train(was_training)
    return gather_shards(shard, N, group)


def gather_shards(shard, n, group=None):
    """Equal row shards (rank r holds rows [r*per, (r+1)*per)) -> the first n rows on every rank:
    one all_gather_into_tensor."""
    world, _ = _world(group)
    if world == 1:
        return shard[:n]
    full = torch.empty((shard.shape[0] * world,) + tuple(shard.shape[1:]), dtype=shard.dtype, device=shard.device)
    dist.all_gather_into_tensor(full, shard.contiguous(), group=group)
    return full[:n]


def score_ragged(table, user, cand_ids, cand_seg, seg_base, out=None, mode=L.SCORE_SIGMOID):
    """out[c] = sigmoid(table[cand_ids[c]] . user[cand_seg[c] - seg_base] / sqrt(H))."""
    n = cand_ids.numel()
    H = table.shape[1]
    for t, name in ((table, "table"), (user, "user")):
        if t.dtype != torch.float32 or not t.is_cuda or t.stride(-1) != 1 or t.dim() != 2:
            raise L.HipError("score_ragged: %s must be a row-major 2-D float32 CUDA tensor" % name)
    if user.shape[1] != H:
        raise L.HipError("score_ragged: user width %d != table width %d" % (user.shape[1], H))
    if cand_ids.dtype != torch.int64 or cand_seg.dtype != torch.int32 or cand_seg.numel() != n:
        raise L.HipError("score_ragged: cand_ids int64 [n] and cand_seg int32 [n] expected")
    cand_ids, cand_seg = cand_ids.contiguous(), cand_seg.contiguous()
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=table.device)
    status = torch.zeros(1, dtype=torch.int32, device=table.device)
    L.call("nr_score_ragged", L.ptr(table), table.stride(0), table.shape[0], L.ptr(cand_ids), L.ptr(cand_seg),
           int(seg_base), n, L.ptr(user), user.stride(0), user.shape[0], H, mode, L.ptr(out), L.ptr(status),
           L.stream_ptr(table))
    return out, status


@torch.no_grad()
def user_reprs(model, table, batch, history_from_table=True, cache=None):
    """User representations [B, H] of a MINDStore.eval_batch.  history_from_table: the history
    news representations are the table's rows; an MHA user encoder then reads its key / value
    projections of the TABLE (computed once per table, kept in ``cache``) through the attention
    kernel's row indirection instead of projecting B*N gathered rows."""
    if not history_from_table:
        user = model.encode_user(batch)[0]
    else:
        enc = model.encoderU
        B, NH = batch["his_id"].shape
        if hasattr(enc, "forward_rows"):
            cache = {} if cache is None else cache
            if cache.get("Y") is None:
                cache["Y"] = enc.project_rows(table)
            user = enc.forward_rows(cache["Y"], batch["his_id"], batch["his_mask"], B, NH)
        else:
            his = K.gather_rows(table, batch["his_id"].reshape(-1).contiguous()).view(B, NH, -1)
            user = model._user_from_his(his, batch)
    user = user.reshape(user.shape[0], -1)
    if user.stride(-1) != 1 or user.stride(0) != user.shape[1]:
        user = user.contiguous()
    return user


@torch.no_grad()
def predict_fast_batch(model, batch, history_from_table=True, cache=None):
    """TwoTowerBaseModel.predict_fast (:78-83) for a batch of impression chunks from
    MINDStore.eval_batch: user representations for the chunks, then the ragged scorer over all
    their candidates.  -> sigmoid scores [n] aligned with batch["cdd_id"]."""
    table = model.news_reprs.weight
    user = user_reprs(model, table, batch, history_from_table, cache)
    preds, _ = score_ragged(table, user, batch["cdd_id"], batch["cand_seg"], batch["chunk0"])
    return preds


@torch.no_grad()
def eval_fast(model, store, batch_impr=1024, group=None, history_from_table=True, news_table=None):
    """Manager._eval_fast (:474-541): -> (preds, labels, grp_off) for the whole split on rank 0
    (packed, device tensors; labels None for test), (None, None, None) on other ranks."""
    world, rank = _world(group)
    was_training = model.training
    model.eval()
    if news_table is None:
        news_table = encode_news_table(model, store, group=group)
    model.init_embedding(news_table)
    c_lo, c_hi = _chunk_range(len(store), world, rank)
    o_lo, o_hi = int(store.cand_off_host[c_lo]), int(store.cand_off_host[c_hi])
    preds = torch.empty(o_hi - o_lo, dtype=torch.float32, device=store.device)
    cache = {}
    for c0 in range(c_lo, c_hi, batch_impr):
        b = min(batch_impr, c_hi - c0)
        x = store.eval_batch(c0, b, with_tokens=not history_from_table)
        o0, o1 = x["cand_range"]
        table = model.news_reprs.weight
        user = user_reprs(model, table, x, history_from_table, cache)
        score_ragged(table, user, x["cdd_id"], x["cand_seg"], c0, out=preds[o0 - o_lo:o1 - o_lo])
    model.destroy_embedding()
    model.train(was_training)
    if world > 1:
        rng = [_chunk_range(len(store), world, r) for r in range(world)]
        sizes = [int(store.cand_off_host[h] - store.cand_off_host[l]) for l, h in rng]
        preds = gather_ranges(preds, sizes, group)
        if preds is None:
            return None, None, None
    return preds, store.cand_labels, store.grp_off


def gather_ranges(local, sizes, group=None):
    """Ranks hold consecutive ranges of one packed vector (rank r: sizes[r] entries): one padded
    all_gather_into_tensor (RCCL on GPUs, gloo on CPUs) -> the whole vector on rank 0, None on
    the other ranks (replaces all_gather_object of Python lists, Manager.py:522-535)."""
    world, rank = _world(group)
    if local.numel() != sizes[rank]:
        raise ValueError("rank %d holds %d entries, sizes says %d" % (rank, local.numel(), sizes[rank]))
    cap = max(max(sizes), 1)
    buf = torch.zeros(cap, dtype=local.dtype, device=local.device)
    buf[:local.numel()] = local
    allp = torch.empty(cap * world, dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(allp, buf, group=group)
    if rank != 0:
        return None
    return torch.cat([allp[r * cap:r * cap + sizes[r]] for r in range(world)])


def _parse_metrics(metrics):
    """Manager.py:1279-1345 metric names -> (wants, ndcg ks, hit ks)."""
    wants, nd, hit = [], [], []
    for m in metrics:
        if m in ("auc", "mean_mrr"):
            wants.append((m, None))
        elif m.startswith("ndcg") or m.startswith("hit"):
            ks = m.split("@")
            lst = [int(t) for t in ks[1].split(";")] if len(ks) > 1 else [1, 2]
            kind = "ndcg" if m.startswith("ndcg") else "hit"
            for k in lst:
                wants.append((kind, k))
                (nd if kind == "ndcg" else hit).append(k)
        elif m in ("rmse", "logloss", "acc", "f1"):
            raise ValueError("metric {0} is a flat (ungrouped) metric; the grouped device path computes "
                             "auc, mean_mrr, ndcg@k and hit@k".format(m))
        else:
            raise ValueError("not define this metric {0}".format(m))
    return wants, sorted(set(nd) | set(hit))


def cal_metric_packed(preds, labels, grp_off, metrics):
    """cal_metric (Manager.py:1276-1345) over packed groups: preds fp32 [n], labels int [n], group
    offsets int64 [G+1] (device tensors).  Per-group terms on the GPU, then np.mean and round(4)
    on the host exactly as the reference."""
    wants, ks = _parse_metrics(metrics)
    if len(ks) > 8:
        raise ValueError("at most 8 distinct cutoffs k per call")
    dev = preds.device
    G = grp_off.numel() - 1
    if labels.dtype != torch.int32:
        labels = labels.to(torch.int32)
    preds, labels, grp_off = preds.contiguous(), labels.contiguous(), grp_off.to(torch.int64).contiguous()
    if preds.dtype != torch.float32:
        preds = preds.float()
    ks_t = torch.tensor(ks if ks else [1], dtype=torch.int32, device=dev)
    W = 2 + 2 * len(ks)
    out = torch.empty(max(G, 1), W, dtype=torch.float64, device=dev)
    flags = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
    L.call("nr_impression_metrics", L.ptr(preds), L.ptr(labels), L.ptr(grp_off), G, L.ptr(ks_t), len(ks),
           L.ptr(out), L.ptr(flags), L.stream_ptr(preds))
    per = out[:G].cpu().numpy()
    fl = flags[:G].cpu().numpy()
    res = {}
    for kind, k in wants:
        if kind == "auc":
            if (fl & L.METRIC_ONE_CLASS).any():
                raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
            if (fl & L.METRIC_NONBINARY).any():
                raise ValueError("multiclass format is not supported")
            res["auc"] = round(np.mean(per[:, 0]), 4)
        elif kind == "mean_mrr":
            res["mean_mrr"] = round(np.mean(per[:, 1]), 4)
        elif kind == "ndcg":
            res["ndcg@{0}".format(k)] = round(np.mean(per[:, 2 + ks.index(k)]), 4)
        else:
            res["hit@{0}".format(k)] = round(np.mean(per[:, 2 + len(ks) + ks.index(k)]), 4)
    return res


def cal_metric(labels, preds, metrics, device="cuda"):
    """cal_metric(labels, preds, metrics) with the reference's signature (Manager.py:1276):
    labels / preds are lists of per-impression lists.  Packs them and runs on the GPU."""
    sizes = [len(p) for p in preds]
    if [len(l) for l in labels] != sizes:
        raise ValueError("labels and preds differ in shape")
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    p = torch.tensor([v for x in preds for v in x], dtype=torch.float32, device=device)
    y = torch.tensor([int(v) for x in labels for v in x], dtype=torch.int32, device=device)
    return cal_metric_packed(p, y, torch.from_numpy(off).to(device), metrics)


def evaluate(model, store, metrics=("auc", "mean_mrr", "ndcg@5;10"), batch_impr=1024, group=None,
             history_from_table=True):
    """Manager.evaluate (:544-590) with fast=True on a dev split: the metrics dict on rank 0,
    None elsewhere."""
    if store.mode != "dev":
        raise ValueError("evaluate needs a dev split with labels")
    preds, labels, grp_off = eval_fast(model, store, batch_impr, group, history_from_table)
    if preds is None:
        return None
    return cal_metric_packed(preds, labels, grp_off, list(metrics))



# ---------------------------------------------------------------- prediction.txt (Manager.py:842-850)
def _check_ragged(preds, grp_off, what):
    L.require_gpu(preds, grp_off)
    if preds.dtype != torch.float32 or preds.dim() != 1 or not preds.is_contiguous():
        raise L.HipError("%s: preds must be a contiguous 1-D float32 CUDA tensor" % what)
    if grp_off.dtype != torch.int64 or grp_off.dim() != 1 or not grp_off.is_contiguous() or grp_off.numel() < 1:
        raise L.HipError("%s: grp_off must be a contiguous 1-D int64 CUDA tensor of G + 1 offsets" % what)
    if grp_off.device != preds.device:
        raise L.HipError("%s: preds and grp_off are on different devices" % what)


def rank_ordinal(preds, grp_off, first_line=1):
    """ss.rankdata(1 - np.asarray(pred), method="ordinal") for every impression of a packed score
    vector (Manager.py:845-846): preds fp32 [n], grp_off int64 [G+1] (device tensors) ->
    (rank int32 [n], line_len int64 [G]); line_len[g] is the byte count of line first_line + g of
    prediction.txt.  The key is the f64 value 1.0 - (double)p and equal keys rank by position, as
    the reference's doubles do.  Raises ValueError when a score is NaN (no ordinal rank), HipError
    when a group has more than RANK_MAX_GROUP candidates."""
    _check_ragged(preds, grp_off, "rank_ordinal")
    n, G = preds.numel(), grp_off.numel() - 1
    sizes = grp_off[1:] - grp_off[:-1]
    # the offsets index preds inside the kernel: one host read of (first, last, smallest and largest size)
    probe = torch.stack([grp_off[0], grp_off[-1], sizes.min() if G else grp_off[0] * 0,
                         sizes.max() if G else grp_off[0] * 0]).tolist()
    if probe[0] != 0 or probe[1] != n or probe[2] < 0:
        raise ValueError("rank_ordinal: grp_off is not a CSR offset array over %d scores" % n)
    rank = torch.empty(n, dtype=torch.int32, device=preds.device)
    line_len = torch.empty(G, dtype=torch.int64, device=preds.device)
    status = torch.zeros(1, dtype=torch.int32, device=preds.device)
    L.call("nr_rank_ordinal", L.ptr(preds), L.ptr(grp_off), G, int(first_line), int(probe[3]), L.ptr(rank),
           L.ptr(line_len), L.ptr(status), L.stream_ptr(preds))
    st = int(status.item())
    if st & L.RANK_GROUP_TOO_LARGE:
        raise L.HipError("rank_ordinal: a group exceeds %d candidates" % L.RANK_MAX_GROUP)
    if st & L.RANK_NAN:
        raise ValueError("rank_ordinal: a score is NaN, which has no ordinal rank")
    return rank, line_len


def _line_offsets(line_len):
    """Exclusive prefix sum [G+1] of the line lengths."""
    off = torch.zeros(line_len.numel() + 1, dtype=torch.int64, device=line_len.device)
    torch.cumsum(line_len, 0, out=off[1:])
    return off


def _format(rank, grp_off, line_off, first_line, text, text_bytes):
    G = grp_off.numel() - 1
    if text.numel() < text_bytes:
        raise L.HipError("format_predictions: text buffer of %d bytes for %d" % (text.numel(), text_bytes))
    L.call("nr_format_prediction", L.ptr(rank), L.ptr(grp_off), L.ptr(line_off), G, int(first_line), L.ptr(text),
           int(text_bytes), L.stream_ptr(rank))


def format_predictions(preds, grp_off, first_line=1):
    """The text of prediction.txt for the impressions of a packed score vector, lines numbered
    first_line, first_line + 1, ... (Manager.py:842-850) -> uint8 device tensor (ASCII)."""
    rank, line_len = rank_ordinal(preds, grp_off, first_line)
    line_off = _line_offsets(line_len)
    total = int(line_off[-1].item())
    text = torch.empty(total, dtype=torch.uint8, device=preds.device)
    _format(rank, grp_off, line_off, first_line, text, total)
    return text


def write_predictions(path, preds, grp_off, slab_bytes=64 << 20):
    """Write prediction.txt (Manager.py:837-850) for a packed score vector; -> bytes written.
    The whole vector is ranked first (a NaN raises before the file exists); the text is then formed
    and copied to pinned host memory in slabs of whole lines of at most slab_bytes (one line when
    that line alone is longer), so the device and host buffers stay bounded on MINDlarge's
    ~0.3 GB of text.  Line numbers run 1, 2, ... in group order."""
    if slab_bytes < 1:
        raise ValueError("slab_bytes must be positive")
    rank, line_len = rank_ordinal(preds, grp_off, 1)
    G = line_len.numel()
    line_off = _line_offsets(line_len)
    off = line_off.cpu().numpy()
    slabs, g0 = [], 0
    while g0 < G:
        g1 = int(np.searchsorted(off, off[g0] + slab_bytes, side="right")) - 1
        g1 = min(max(g1, g0 + 1), G)
        slabs.append((g0, g1))
        g0 = g1
    cap = max([int(off[b] - off[a]) for a, b in slabs] + [1])
    text = torch.empty(cap, dtype=torch.uint8, device=preds.device)
    host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
    parent = os.path.dirname(path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    written = 0
    with open(path, "wb") as f:
        for a, b in slabs:
            nb = int(off[b] - off[a])
            _format(rank, grp_off[a:b + 1], line_off[a:b + 1] - line_off[a], 1 + a, text, nb)
            host[:nb].copy_(text[:nb], non_blocking=True)
            torch.cuda.current_stream(preds.device).synchronize()
            f.write(memoryview(host.numpy())[:nb])
            written += nb
    return written


def test(model, store, path, batch_impr=1024, group=None, history_from_table=True):
    """Manager.test (:815-852) with fast=True, minus the checkpoint load: scores the split with
    eval_fast and writes prediction.txt to ``path`` on rank 0 (one line per impression, numbered
    1, 2, ... in order, not by impr_index).  -> path on rank 0, None elsewhere.  Takes test and
    dev stores (a train split has no impressions to rank)."""
    if store.mode not in ("test", "dev"):
        raise ValueError("test needs a test or dev split, not %s" % store.mode)
    preds, _, grp_off = eval_fast(model, store, batch_impr, group, history_from_table)
    if preds is None:
        return None
    write_predictions(path, preds, grp_off)
    return path


# ---------------------------------------------------------------- full-corpus retrieval (--mode recall -rt d)
def topk_news(table, user, k, first_row=1, row_mask=None, exclude=None, n_slices=0):
    """The k best rows of ``table`` [N, H] for every row of ``user`` [U, H], exact (csrc/topk.hip):
    score = table[j] . user[i] / sqrt(H) as score_ragged's raw logits, ordered by score descending
    and, among equal scores, row id ascending.  -> (ids int64 [U, k], scores fp32 [U, k]).

    Eligible rows: j >= first_row (1 skips the padded "" news), row_mask[j] != 0 (uint8 [N], optional)
    and j not in exclude[i] (int64 [U, E], optional; entries outside [0, N) are padding).  With fewer
    than k eligible rows the tail is id -1 / score -inf.  n_slices: launch geometry (0 = automatic);
    the result does not depend on it.  Raises ValueError when an eligible row's score is not finite."""
    L.require_gpu(table, user, row_mask, exclude)
    for t, name in ((table, "table"), (user, "user")):
        if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(-1) != 1):
            raise L.HipError("topk_news: %s must be a row-major 2-D float32 CUDA tensor" % name)
    N, H = table.shape
    U = user.shape[0]
    if user.shape[1] != H:
        raise L.HipError("topk_news: user width %d != table width %d" % (user.shape[1], H))
    if user.device != table.device:
        raise L.HipError("topk_news: table and user are on different devices")
    k = int(k)
    if not 1 <= k <= L.TOPK_MAX_K:
        raise L.HipError("topk_news: k = %d outside [1, %d]" % (k, L.TOPK_MAX_K))
    if row_mask is not None:
        if row_mask.dtype != torch.uint8 or row_mask.dim() != 1 or row_mask.numel() != N:
            raise L.HipError("topk_news: row_mask must be uint8 [%d]" % N)
        row_mask = row_mask.contiguous()
    E = 0
    if exclude is not None:
        if exclude.dtype != torch.int64 or exclude.dim() != 2 or exclude.shape[0] != U:
            raise L.HipError("topk_news: exclude must be int64 [%d, E]" % U)
        E = exclude.shape[1]
        if E > L.TOPK_MAX_EXCLUDE:
            raise L.HipError("topk_news: %d exclude ids per user, at most %d" % (E, L.TOPK_MAX_EXCLUDE))
        exclude = exclude.contiguous() if E else None
    dev = table.device
    ids = torch.empty(U, k, dtype=torch.int64, device=dev)
    scores = torch.empty(U, k, dtype=torch.float32, device=dev)
    if U == 0:
        return ids, scores
    ws_bytes = int(L.load().nr_topk_workspace(U, N, k, int(n_slices)))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("nr_topk_news", L.ptr(table), table.stride(0), N, L.ptr(user), user.stride(0), U, H, k, int(first_row),
           L.ptr(row_mask), L.ptr(exclude), E, int(n_slices), L.ptr(ids), L.ptr(scores), L.ptr(ws), ws_bytes,
           L.ptr(status), L.stream_ptr(table))
    if int(status.item()) & L.TOPK_NONFINITE:
        raise ValueError("topk_news: a non-finite score among the eligible rows")
    return ids, scores


# ---------------------------------------------------------------- sparse recall (--mode recall -rt s)
class BM25Index:
    """The token-level BM25 inverted index of a corpus (csrc/bm25.hip; the definition is in
    include/newsrec_hip.h), as build_bm25_index makes it:

      tok          int32 [R, L]   the corpus (a store's tok: row 0 included)
      post_ids     int32 [V, P]   token -> its P best rows, best first, padded with R
      post_scores  fp64  [V, P]   their BM25 scores, padded with +0.0
      df           int64 [V]      occurrences in columns 1 .. L-1;  idf fp64 [V] (formed on the host)
      fwd, keep    fp32 [R, L], int64 [R] (a bit per column)   the pruned index seen from the news side
      n_rows = R, vocab = V, postings = P, k, special; bad_tokens: a token outside [0, V) was ignored
    """

    def __init__(self, tok, post_ids, post_scores, df, idf, fwd, keep, k, special, bad_tokens=False):
        self.tok, self.post_ids, self.post_scores, self.df, self.idf = tok, post_ids, post_scores, df, idf
        self.fwd, self.keep, self.k, self.special = fwd, keep, int(k), tuple(int(s) for s in special)
        self.n_rows, self.vocab, self.postings = tok.shape[0], post_ids.shape[0], post_ids.shape[1]
        self.bad_tokens = bool(bad_tokens)

    def to_reference(self):
        """The [V, P, 2] float64 CPU tensor of (row, score) pairs that the reference saves as
        inverted_index_bm25.pt (utils.py:234-245)."""
        out = torch.empty(self.vocab, self.postings, 2, dtype=torch.float64)
        out[:, :, 0] = self.post_ids.cpu().to(torch.float64)
        out[:, :, 1] = self.post_scores.cpu()
        return out

    _ARRAYS = ("tok", "post_ids", "post_scores", "df", "idf", "fwd", "keep")

    def save(self, path):
        """np.savez of the arrays and parameters (no pickle).  -> the file written (.npz appended if absent)."""
        path = path if path.endswith(".npz") else path + ".npz"
        arrays = {n: getattr(self, n).cpu().numpy() for n in self._ARRAYS}
        meta = np.array([self.k, int(self.bad_tokens)] + list(self.special), np.int64)
        np.savez(path, meta=meta, **arrays)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            arrays = [torch.from_numpy(z[n]).to(device) for n in cls._ARRAYS]
            meta = [int(v) for v in z["meta"]]
        return cls(*arrays, k=meta[0], special=meta[2:5], bad_tokens=meta[1])


def _check_tokens(t, name, who):
    if t.dtype != torch.int32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(-1) != 1):
        raise L.HipError("%s: %s must be a row-major 2-D int32 CUDA tensor" % (who, name))


def build_bm25_index(tok, vocab=30522, postings=100, k=2, special=(0, 101, 102)):
    """construct_inverted_index(corpus, BM25_token(corpus)) (utils.py:219-246, :287-342) of the corpus
    ``tok`` int32 [R, L] (a store's tok) on the device -> BM25Index.  One small device-to-host copy: the
    idf is formed on the host from the V occurrence counts with math.log, which makes it the reference's
    bit for bit."""
    import math
    L.require_gpu(tok)
    _check_tokens(tok, "tok", "build_bm25_index")
    R, Ls = tok.shape
    vocab, postings, k = int(vocab), int(postings), int(k)
    special = tuple(int(s) for s in special)
    if not 1 <= Ls <= L.BM25_MAX_L:
        raise L.HipError("build_bm25_index: %d columns, at most %d" % (Ls, L.BM25_MAX_L))
    if not 1 <= postings <= L.BM25_MAX_POSTINGS:
        raise L.HipError("build_bm25_index: postings = %d outside [1, %d]" % (postings, L.BM25_MAX_POSTINGS))
    if vocab < 1 or k < 1 or len(special) != 3:
        raise L.HipError("build_bm25_index: vocab and k must be positive and special hold three ids")
    dev = tok.device
    df = torch.empty(vocab, dtype=torch.int64, device=dev)
    n_post = torch.empty(vocab, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    S = L.stream_ptr(tok)
    L.call("nr_bm25_count", L.ptr(tok), tok.stride(0), R, Ls, vocab, *special, L.ptr(df), L.ptr(n_post), L.ptr(status),
           S)
    idf = torch.tensor([math.log((R - d + 0.5) / (d + 0.5) + 1) if d > 0 else 0.0 for d in df.cpu().tolist()],
                       dtype=torch.float64).to(dev)
    post_ids = torch.empty(vocab, postings, dtype=torch.int32, device=dev)
    post_scores = torch.empty(vocab, postings, dtype=torch.float64, device=dev)
    ws_bytes = int(L.load().nr_bm25_build_workspace(R, Ls, vocab))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    L.call("nr_bm25_build", L.ptr(tok), tok.stride(0), R, Ls, vocab, postings, k, *special, L.ptr(idf), L.ptr(n_post),
           L.ptr(post_ids), L.ptr(post_scores), L.ptr(ws), ws_bytes, S)
    fwd = torch.empty(R, Ls, dtype=torch.float32, device=dev)
    keep = torch.empty(R, dtype=torch.int64, device=dev)
    L.call("nr_bm25_forward", L.ptr(tok), tok.stride(0), R, Ls, vocab, postings, L.ptr(post_ids), L.ptr(post_scores),
           L.ptr(fwd), Ls, L.ptr(keep), S)
    bad = bool(int(status.item()) & L.BM25_BAD_TOKEN)
    return BM25Index(tok, post_ids, post_scores, df, idf, fwd, keep, k, special, bad)


def sparse_topk_news(index, query_tokens, k, first_row=1, row_mask=None, exclude=None, n_slices=0):
    """The k best rows of a BM25Index for every row of ``query_tokens`` int32 [U, Tq] (a bag of tokens per
    user; specials, out-of-range values and repeats are harmless), exact (csrc/bm25.hip): score = the fp32
    sum, in column order, of the row's kept postings whose token the user holds; a row with no such
    posting is not returned.  first_row, row_mask, exclude, the order, the -1 / -inf tail and n_slices as
    topk_news.  -> (ids int64 [U, k], scores fp32 [U, k])."""
    L.require_gpu(index.tok, query_tokens, row_mask, exclude)
    _check_tokens(query_tokens, "query_tokens", "sparse_topk_news")
    R, Ls = index.tok.shape
    U, Tq = query_tokens.shape
    dev = index.tok.device
    if query_tokens.device != dev:
        raise L.HipError("sparse_topk_news: index and query_tokens are on different devices")
    k = int(k)
    if not 1 <= k <= L.TOPK_MAX_K:
        raise L.HipError("sparse_topk_news: k = %d outside [1, %d]" % (k, L.TOPK_MAX_K))
    if row_mask is not None:
        if row_mask.dtype != torch.uint8 or row_mask.dim() != 1 or row_mask.numel() != R:
            raise L.HipError("sparse_topk_news: row_mask must be uint8 [%d]" % R)
        row_mask = row_mask.contiguous()
    E = 0
    if exclude is not None:
        if exclude.dtype != torch.int64 or exclude.dim() != 2 or exclude.shape[0] != U:
            raise L.HipError("sparse_topk_news: exclude must be int64 [%d, E]" % U)
        E = exclude.shape[1]
        if E > L.TOPK_MAX_EXCLUDE:
            raise L.HipError("sparse_topk_news: %d exclude ids per user, at most %d" % (E, L.TOPK_MAX_EXCLUDE))
        exclude = exclude.contiguous() if E else None
    ids = torch.empty(U, k, dtype=torch.int64, device=dev)
    scores = torch.empty(U, k, dtype=torch.float32, device=dev)
    if U == 0:
        return ids, scores
    ws_bytes = int(L.load().nr_bm25_topk_workspace(U, R, k, int(n_slices)))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    L.call("nr_bm25_topk", L.ptr(query_tokens), max(query_tokens.stride(0), Tq), U, Tq, L.ptr(index.tok),
           index.tok.stride(0), L.ptr(index.fwd), index.fwd.stride(0), L.ptr(index.keep), R, Ls, index.vocab,
           *index.special, k, int(first_row), L.ptr(row_mask), L.ptr(exclude), E, int(n_slices), L.ptr(ids),
           L.ptr(scores), L.ptr(ws), ws_bytes, L.stream_ptr(index.tok))
    return ids, scores


def history_tokens(store, his_id, his_mask):
    """The query of sparse recall: the tokens of every user's history, int32 [U, his_size * L] =
    store.tok[his_id] with the masked history slots set to pad (0).  Plain torch."""
    U = his_id.shape[0]
    t = store.tok[his_id.reshape(U, -1).long()]
    t = t * (his_mask.reshape(U, -1, 1) != 0).to(t.dtype)
    return t.reshape(U, -1).contiguous()


def merge_recall(ids_a, ids_b):
    """The "sd" merge of two recall lists [U, Ka], [U, Kb] (best first, -1 = no entry): round robin
    a0, b0, a1, b1, ..., dropping -1 entries and ids already taken, compacted to the front and padded
    with -1.  -> int64 [U, Ka + Kb].  Plain torch on the inputs' device (CPU tensors work)."""
    if ids_a.dim() != 2 or ids_b.dim() != 2 or ids_a.shape[0] != ids_b.shape[0]:
        raise ValueError("merge_recall takes two [U, K] id tensors with the same U")
    U, (ka, kb) = ids_a.shape[0], (ids_a.shape[1], ids_b.shape[1])
    W = max(ka, kb)
    wide = [torch.nn.functional.pad(t.to(torch.int64), (0, W - t.shape[1]), value=-1) for t in (ids_a, ids_b)]
    x = torch.stack(wide, 2).reshape(U, 2 * W)
    vals, idx = torch.sort(x, dim=1, stable=True)           # equal ids stay in round-robin order
    later = torch.zeros_like(vals, dtype=torch.bool)
    later[:, 1:] = vals[:, 1:] == vals[:, :-1]
    dup = torch.zeros_like(later).scatter_(1, idx, later)
    valid = (x >= 0) & ~dup
    front = torch.sort((~valid).to(torch.int8), dim=1, stable=True).indices
    return torch.where(valid, x, torch.full_like(x, -1)).gather(1, front)[:, :ka + kb]


@torch.no_grad()
def recommend(model, store, k=10, batch_impr=1024, candidates="impressed", exclude_history=True, news_table=None,
              recall_type="d", bm25=None):
    """Recall over a dev or test split: the k best news of the WHOLE table for every impression's
    user, one row per impression (not per chunk).  -> (ids int64 [n_impr, k], scores fp32 [n_impr, k]),
    n_impr = len(store.grp_off_host) - 1.

    The store is walked in eval_batch batches of ``batch_impr`` chunks; an impression cut into several
    chunks shares its history, so its first chunk (store.first_chunk_host) gives its user
    (user_reprs with history_from_table).  candidates: "impressed" searches the rows that occur in
    store.cand_ids (the reference's news_set, construct_cddidx_for_recall, Manager.py:1089-1113), "all"
    every row except the padded row 0.  exclude_history: the impression's own history is not recommended.
    news_table: an encode_news_table result to reuse.  Single process: the impressions are not sharded
    over ranks (no ``group`` argument).

    recall_type (the reference's -rt, Manager.py:52): "d" dense (topk_news over the encoded table), "s"
    sparse (sparse_topk_news of the history's tokens over ``bm25``, a BM25Index of store.tok, built here
    when None; the model is not used), "sd" both: merge_recall(sparse, dense) ids [n_impr, 2k], scores None."""
    if store.mode not in ("dev", "test"):
        raise ValueError("recommend needs a dev or test split, not %s" % store.mode)
    if candidates not in ("impressed", "all"):
        raise ValueError("candidates must be 'impressed' or 'all'")
    if recall_type not in ("d", "s", "sd"):
        raise ValueError("recall_type must be 'd', 's' or 'sd'")
    dense, sparse = "d" in recall_type, "s" in recall_type
    dev, n_rows = store.tok.device, store.tok.shape[0]
    if dense:
        was_training = model.training
        model.eval()
        table = news_table if news_table is not None else encode_news_table(model, store)
        dev, n_rows = table.device, table.shape[0]
    if sparse:
        index = bm25 if bm25 is not None else build_bm25_index(store.tok)
        if index.n_rows != store.tok.shape[0]:
            raise ValueError("bm25 indexes %d rows, the store has %d" % (index.n_rows, store.tok.shape[0]))
    mask = None
    if candidates == "impressed":
        mask = torch.zeros(n_rows, dtype=torch.uint8, device=dev)
        mask[store.cand_ids] = 1
    first = store.first_chunk_host
    n_impr = len(first)
    out = {t: (torch.empty(n_impr, k, dtype=torch.int64, device=dev),
               torch.empty(n_impr, k, dtype=torch.float32, device=dev)) for t in recall_type}
    cache = {}
    for c0 in range(0, len(store), batch_impr):
        b = min(batch_impr, len(store) - c0)
        i0, i1 = np.searchsorted(first, [c0, c0 + b])
        if i0 == i1:
            continue
        x = store.eval_batch(c0, b)
        rows = torch.from_numpy(first[i0:i1] - c0).to(dev)
        sub = {key: x[key][rows] for key in ("impr_index", "user_id", "his_id", "his_mask")}
        his = sub["his_id"].reshape(i1 - i0, -1) if exclude_history else None
        if dense:
            user = user_reprs(model, table, sub, True, cache)
            out["d"][0][i0:i1], out["d"][1][i0:i1] = topk_news(table, user, k, first_row=1, row_mask=mask, exclude=his)
        if sparse:
            query = history_tokens(store, sub["his_id"], sub["his_mask"])
            out["s"][0][i0:i1], out["s"][1][i0:i1] = sparse_topk_news(index, query, k, first_row=1, row_mask=mask,
                                                                      exclude=his)
    if dense:
        model.train(was_training)
    if recall_type == "sd":
        return merge_recall(out["s"][0], out["d"][0]), None
    return out[recall_type]


def recall_metrics(top_ids, store, ks=(5, 10)):
    """hit_score-style retrieval metrics (Manager.py:1240-1255) of ``top_ids`` [n_impr, K] (recommend's
    ids, best first) against the clicks of a dev split: over the impressions with at least one clicked
    candidate (store.cand_labels == 1, grouped by store.grp_off),
      recall@k = |clicked ∩ top-k| / |clicked|,   hit@k = 1 if any clicked candidate is in the top-k,
    averaged and rounded to 4 places as cal_metric does; "n_impr_scored" counts those impressions.
    Plain torch on the device the inputs are on (CPU tensors work)."""
    if store.cand_labels is None:
        raise ValueError("recall_metrics needs a dev split with labels")
    dev = top_ids.device
    grp_off = store.grp_off.to(dev, torch.int64)
    G = grp_off.numel() - 1
    if top_ids.dim() != 2 or top_ids.shape[0] != G:
        raise ValueError("top_ids must be [%d, K], one row per impression" % G)
    if max(ks) > top_ids.shape[1] or min(ks) < 1:
        raise ValueError("ks must lie in [1, %d]" % top_ids.shape[1])
    cand = store.cand_ids.to(dev, torch.int64)
    sizes = grp_off[1:] - grp_off[:-1]
    seg = torch.repeat_interleave(torch.arange(G, device=dev), sizes)
    clicked = store.cand_labels.to(dev) == 1
    # distinct (impression, clicked news) pairs: a news listed twice counts once
    span = int(cand.max().item()) + 1 if cand.numel() else 1
    pairs = torch.unique(seg[clicked] * span + cand[clicked])
    g, nid = pairs // span, pairs % span
    n_click = torch.bincount(g, minlength=G)
    scored = n_click > 0
    res = {}
    for k in ks:
        found = (top_ids[g, :k] == nid[:, None]).any(1)
        n_hit = torch.bincount(g, weights=found.to(torch.float64), minlength=G)
        rec = (n_hit[scored] / n_click[scored].to(torch.float64)).cpu().numpy()
        hit = (n_hit[scored] > 0).to(torch.float64).cpu().numpy()
        res["recall@{0}".format(k)] = round(float(np.mean(rec)), 4) if rec.size else 0.0
        res["hit@{0}".format(k)] = round(float(np.mean(hit)), 4) if hit.size else 0.0
    res["n_impr_scored"] = int(scored.sum().item())
    return res
