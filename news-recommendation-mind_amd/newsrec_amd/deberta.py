"""The DeBERTa tower of PLM's ``-b deberta`` (models/PLM.py:19-28) on the HIP kernels.

``DebertaModel`` mirrors transformers' DebertaModel as microsoft/deberta-base configures it
(relative_attention, pos_att_type c2p | p2c, max_relative_positions -1 -> K = max_position_embeddings,
position_biased_input False, type_vocab_size 0, layer_norm_eps 1e-7, exact GELU, no pooler, no talking
heads), with its module tree and ``state_dict`` names, shapes and order, so checkpoints load unchanged.
Pretrained weights are not available offline: the default is transformers' random init (normal(0, 0.02),
zero biases including q_bias / v_bias, unit LayerNorms).

Like BertModel the whole encoder is ONE autograd.Function (``DebertaFn``) over several token segments
at once; it shares BertFn's layer body behind the attention core (bert.layer_tail_fwd / _bwd).  With m the
attention mask and L <= 64 tokens per title:

  x   = Dropout(m * LN(word[ids]))           nr_bert_embed_fwd on zero position / type rows, then the mask
per layer
  qkv = x in_projᵀ + (q_bias | 0 | v_bias)   nr_gemm_f32 (N = 3H, head h owns columns [192 h, 192 h + 192))
  rel = Dropout(rel_embeddings[K-L : K+L])   2L rows (torch ops on the counter RNG's keep mask)
  pk  = rel pos_projᵀ, pq = rel pos_q_projᵀ + b          nr_gemm_f32, M = 2L
  ctx = disentangled attention(qkv, pk, pq, m)           nr_deb_attn_fwd
  ...   bert.layer_tail_fwd: dense + dropout + residual LN, GELU FFN, dense + dropout + residual LN

Dropout counters.  One training forward takes ONE range of the model's counter stream (one nr_rng_take), laid
out as 1 + 4 x layers sites over the rows T = sum nseq L of all segments:
  embeddings [T H] (segment at row r0: key offset site + r0 H, element t H + c of the local row t);
  then per layer
    relative rows: sum over segments of 2L H  (segment g: key offset site + sum of the earlier segments'
                   2L H, element r H + c of the 2L x H slice),
    attention probabilities: sum over segments of nseq heads L L  (segment g: key offset site + the earlier
                   segments' counts, element ((s heads + h) L + i) L + j: nr_deb_attn_fwd's layout),
    attention-output dense [T H], FFN-output dense [T H]  (key offset site, element t H + c of the global row).
tests/deberta_util.DebertaDropout restates this layout and replays every mask.
"""
from collections import namedtuple

import torch
from torch import nn

from . import _lib as L
from . import kernels as K
from .bert import _Segment, layer_tail_bwd, layer_tail_fwd
from .functions import _empty, _gemm_backward, _proj_wgrad, _zeros_views, table_grad_buffer

DEB_MAX_L = K.DEB_MAX_L


class DebertaConfig:
    """transformers.DebertaConfig as microsoft/deberta-base sets it."""

    def __init__(self, vocab_size=50265, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, max_position_embeddings=512, layer_norm_eps=1e-7,
                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, pad_token_id=0, initializer_range=0.02):
        self.vocab_size = vocab_size
        self.hidden_size = hidden_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.intermediate_size = intermediate_size
        self.max_position_embeddings = max_position_embeddings     # K: rel_embeddings has 2K rows
        self.layer_norm_eps = layer_norm_eps
        self.hidden_dropout_prob = hidden_dropout_prob
        self.attention_probs_dropout_prob = attention_probs_dropout_prob
        self.pad_token_id = pad_token_id
        self.initializer_range = initializer_range
        self.attention_type = "deberta"


DebertaOutput = namedtuple("DebertaOutput", ["last_hidden_state"])


class DebertaEmbeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size, padding_idx=c.pad_token_id)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class DisentangledSelfAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        H = c.hidden_size
        self.q_bias = nn.Parameter(torch.zeros(H))
        self.v_bias = nn.Parameter(torch.zeros(H))
        self.in_proj = nn.Linear(H, 3 * H, bias=False)
        self.pos_proj = nn.Linear(H, H, bias=False)
        self.pos_q_proj = nn.Linear(H, H)
        self.pos_dropout = nn.Dropout(c.hidden_dropout_prob)
        self.dropout = nn.Dropout(c.attention_probs_dropout_prob)


class DebertaSelfOutput(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class DebertaAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.self = DisentangledSelfAttention(c)
        self.output = DebertaSelfOutput(c)


class DebertaIntermediate(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.intermediate_size)


class DebertaLayerOutput(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.intermediate_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class DebertaLayer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = DebertaAttention(c)
        self.intermediate = DebertaIntermediate(c)
        self.output = DebertaLayerOutput(c)


class DebertaEncoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([DebertaLayer(c) for _ in range(c.num_hidden_layers)])
        self.rel_embeddings = nn.Embedding(2 * c.max_position_embeddings, c.hidden_size)


def _i64(c):
    """A 64-bit constant as the int64 of the same bits."""
    return c - (1 << 64) if c >= 1 << 63 else c


def _srl(z, n):
    return (z >> n) & ((1 << (64 - n)) - 1)


def counter_keep(rng, offsets, n, p):
    """The counter RNG's keep masks (csrc/common.h nr_dropout_key / nr_dropout_keep) in torch ops, for tensors
    too small to earn a kernel: rng the device (seed, offset) snapshot, offsets [m] int64 added to its offset
    -> bool [m, n], row k the keep bits of elements 0 .. n-1 under key (seed, offset + offsets[k]).  Integer
    arithmetic in int64 (products wrap; the low 32 bits are what the hash keeps)."""
    z = rng[0] * _i64(0x9E3779B97F4A7C15) + (rng[1] + offsets) * _i64(0xD1B54A32D192ED03) + _i64(0x632BE59BD9B4E019)
    z = (z ^ _srl(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _srl(z, 27)) * _i64(0x94D049BB133111EB)
    key = _srl(z ^ _srl(z, 31), 32)
    e = torch.arange(n, device=rng.device, dtype=torch.int64)
    x = (key[:, None] + e[None, :] * 0x9E3779B1) & 0xFFFFFFFF
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF
    x = ((x ^ (x >> 15)) * 0x846CA68B) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    t = float(torch.tensor(p, dtype=torch.float32)) * 4294967296.0
    return x >= (0xFFFFFFFF if t >= 4294967295.0 else int(t))


N_EMB, N_LAYER = 3, 16      # tensors of the embeddings and of one layer in DebertaFn's flat parameter list


class DebertaFn(torch.autograd.Function):
    """The DebertaModel forward over concatenated segments -> last_hidden [T, H].
    ``drop`` = None (eval / p = 0) or (seed, offset, rng, sites): the range's snapshot and the start of each of
    its 1 + 4 x layers sites inside it."""

    @staticmethod
    def forward(ctx, cfg, segs, drop, *params):
        ctx.prec = K.get_gemm_precision()
        c = cfg
        H, heads, nl, KP = c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.max_position_embeddings
        word, elw, elb = params[:N_EMB]
        lp = [params[N_EMB + N_LAYER * i: N_EMB + N_LAYER * (i + 1)] for i in range(nl)]
        rel_emb = params[N_EMB + N_LAYER * nl]
        dev = word.device
        T = sum(s.nseq * s.L for s in segs)
        r0s, r = [], 0
        for s in segs:
            r0s.append(r)
            r += s.nseq * s.L
        p_h = c.hidden_dropout_prob if drop is not None else 0.0
        p_a = c.attention_probs_dropout_prob if drop is not None else 0.0

        def site(k, p, extra=0):
            if drop is None or p <= 0.0:
                return dict(p_drop=0.0)
            seed, off, rng, sites = drop
            return dict(p_drop=p, seed=seed, offset=sites[k] + extra, rng=rng)

        # per segment: where its relative rows / probabilities start inside their sites
        rel0, att0, ra, aa = [], [], 0, 0
        for s in segs:
            rel0.append(ra)
            att0.append(aa)
            ra += 2 * s.L * H
            aa += s.nseq * heads * s.L * s.L

        Lmax = max(s.L for s in segs)
        zpos = torch.zeros(Lmax + 1, H, device=dev)            # no position or type embeddings: zero rows
        x = _empty(T, H, word)
        st_e = torch.empty(T, 2, device=dev)
        for s, r0 in zip(segs, r0s):
            K.bert_embed_fwd(word, zpos, zpos[Lmax], s.ids, s.nseq, s.L, elw, elb, c.layer_norm_eps,
                             x[r0:r0 + s.nseq * s.L], st_e[r0:r0 + s.nseq * s.L], **site(0, p_h, r0 * H))
        maskf = torch.cat([s.mask.reshape(-1) for s in segs]).ne(0).to(torch.float32).unsqueeze(1)
        x.mul_(maskf)
        saved, rel_saved = [], []
        rel_keeps = None
        if p_h > 0.0:
            # every layer's keep mask of a segment's 2L relative rows in one pass: the layers' sites are one
            # stride apart
            sites = drop[3]
            layer_offs = torch.arange(nl, device=dev, dtype=torch.int64) * (sites[5] - sites[1] if nl > 1 else 0)
            rel_keeps = [counter_keep(drop[2], layer_offs + (sites[1] + rel0[g]), 2 * s.L * H, p_h).view(nl, 2 * s.L, H)
                         for g, s in enumerate(segs)]
        for li, w in enumerate(lp):
            qb, vb, win, wpk, wpq, bpq = w[:6]
            bqkv = torch.stack([qb.view(heads, 64), torch.zeros_like(qb).view(heads, 64), vb.view(heads, 64)],
                               1).reshape(3 * H)
            qkv = _empty(T, 3 * H, word)
            K.gemm(T, 3 * H, H, K.operand(x, L.KCONTIG), K.operand(win, L.KCONTIG), qkv, bias=bqkv)
            keeps = [k[li] for k in rel_keeps] if rel_keeps is not None else None
            cx = _empty(T, H, word)
            probs = torch.empty(max(aa, 1), device=dev)
            per_seg = []
            for g, (s, r0) in enumerate(zip(segs, r0s)):
                n = s.nseq * s.L
                rel = rel_emb[KP - s.L: KP + s.L]
                if keeps is not None:
                    rel = rel * keeps[g] * (1.0 / (1.0 - p_h))
                pk = _empty(2 * s.L, H, word)
                pq = _empty(2 * s.L, H, word)
                K.gemm(2 * s.L, H, H, K.operand(rel, L.KCONTIG), K.operand(wpk, L.KCONTIG), pk)
                K.gemm(2 * s.L, H, H, K.operand(rel, L.KCONTIG), K.operand(wpq, L.KCONTIG), pq, bias=bpq)
                K.deb_attn_fwd(qkv[r0:r0 + n], pk, pq, s.mask, s.nseq, s.L, heads,
                               probs[att0[g]:att0[g] + s.nseq * heads * s.L * s.L], cx[r0:r0 + n],
                               **site(2 + 4 * li, p_a, att0[g]))
                per_seg.append((rel, pk, pq, keeps[g] if keeps is not None else None))
            a, st1, h1, U, G, o, st2, h2 = layer_tail_fwd(c, x, cx, w[6:], site(3 + 4 * li, p_h), site(4 + 4 * li, p_h))
            saved += [x, qkv, cx, probs, a, st1, h1, U, G, o, st2]
            rel_saved.append(per_seg)
            x = h2
        ctx.save_for_backward(*params, st_e, maskf, zpos, *saved)
        ctx.cfg, ctx.segs, ctx.r0s, ctx.att0 = cfg, segs, r0s, att0
        ctx.rel_saved = rel_saved
        ctx.site, ctx.p = site, (p_h, p_a)
        ctx.n_params = len(params)
        return x

    @staticmethod
    @_gemm_backward
    def backward(ctx, dhid):
        c = ctx.cfg
        H, heads, nl, KP = c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.max_position_embeddings
        sv = ctx.saved_tensors
        npar = ctx.n_params
        params = sv[:npar]
        st_e, maskf, zpos = sv[npar:npar + 3]
        saved = sv[npar + 3:]
        word, elw, elb = params[:N_EMB]
        lp = [params[N_EMB + N_LAYER * i: N_EMB + N_LAYER * (i + 1)] for i in range(nl)]
        rel_emb = params[N_EMB + N_LAYER * nl]
        dev = word.device
        T = st_e.shape[0]
        segs, r0s, att0, site = ctx.segs, ctx.r0s, ctx.att0, ctx.site
        p_h, p_a = ctx.p
        grads = [None] * npar
        drel_emb = torch.zeros_like(rel_emb)

        dh = _empty(T, H, word)
        dh.copy_(dhid)
        for li in reversed(range(nl)):
            x, qkv, cx, probs, a, st1, h1, U, G, o, st2 = saved[11 * li: 11 * (li + 1)]
            w = lp[li]
            win, wpk, wpq = w[2], w[3], w[4]
            # one fill for the layer's gradients; q_bias / v_bias are slices of the fused [3H] bias gradient
            dbqkv, *g = _zeros_views(dev, (3 * H,), *[tuple(t.shape) for t in w[2:]])
            dx, dcx = layer_tail_bwd(dh, x, cx, (a, st1, h1, U, G, o, st2), w[6:], g[4:],
                                     site(3 + 4 * li, p_h), site(4 + 4 * li, p_h))
            dqkv = _empty(T, 3 * H, word)
            for gi, (s, r0) in enumerate(zip(segs, r0s)):
                n = s.nseq * s.L
                rel, pk, pq, keep = ctx.rel_saved[li][gi]
                dpk = _empty(2 * s.L, H, word)
                dpq = _empty(2 * s.L, H, word)
                K.deb_attn_bwd(qkv[r0:r0 + n], pk, pq, s.mask, s.nseq, s.L, heads,
                               probs[att0[gi]:att0[gi] + s.nseq * heads * s.L * s.L], dcx[r0:r0 + n],
                               dqkv[r0:r0 + n], dpk, dpq, **site(2 + 4 * li, p_a, att0[gi]))
                # through the two position projections to the 2L rows of rel_embeddings
                drel = _empty(2 * s.L, H, word)
                K.gemm(2 * s.L, H, H, K.operand(dpk, L.KCONTIG), K.operand(wpk, L.MNCONTIG), drel)
                K.gemm(2 * s.L, H, H, K.operand(dpq, L.KCONTIG), K.operand(wpq, L.MNCONTIG), drel,
                       epilogue=L.EPI_ACCUM)
                _proj_wgrad(dpk, K.operand(rel, L.MNCONTIG), g[1], None, 2 * s.L)
                _proj_wgrad(dpq, K.operand(rel, L.MNCONTIG), g[2], g[3], 2 * s.L)
                if keep is not None:
                    drel = drel * keep * (1.0 / (1.0 - p_h))
                drel_emb[KP - s.L: KP + s.L] += drel
            K.gemm(T, H, 3 * H, K.operand(dqkv, L.KCONTIG), K.operand(win, L.MNCONTIG), dx, epilogue=L.EPI_ACCUM)
            _proj_wgrad(dqkv, K.operand(x, L.MNCONTIG), g[0], dbqkv, T)
            db = dbqkv.view(heads, 3, 64)
            base = N_EMB + N_LAYER * li
            grads[base], grads[base + 1] = db[:, 0].reshape(H), db[:, 2].reshape(H)
            for k in range(N_LAYER - 2):
                grads[base + 2 + k] = g[k]
            dh = dx
        dh.mul_(maskf)
        ds = _empty(T, H, word)
        delw, delb = _zeros_views(dev, tuple(elw.shape), tuple(elb.shape))
        Lmax = zpos.shape[0] - 1
        ids_all = []
        for s, r0 in zip(segs, r0s):
            n = s.nseq * s.L
            K.bert_embed_bwd(word, zpos, zpos[Lmax], s.ids, s.nseq, s.L, elw, st_e[r0:r0 + n], dh[r0:r0 + n],
                             ds[r0:r0 + n], delw, delb, **site(0, p_h, r0 * H))
            ids_all.append(s.ids)
        dword = table_grad_buffer(word, word.shape[0], word.shape[1], dev, zero=True)
        K.embedding_bwd(ds, torch.cat(ids_all) if len(ids_all) > 1 else ids_all[0], dword,
                        padding_idx=c.pad_token_id)
        grads[:N_EMB] = [dword, delw, delb]
        grads[N_EMB + N_LAYER * nl] = drel_emb
        return (None, None, None) + tuple(grads)


class DebertaModel(nn.Module):
    """transformers.DebertaModel (deberta-base's configuration) on the HIP kernels: ``model(ids, mask)`` and
    ``encode_segments`` return ``last_hidden_state`` (the model has no pooler; PLM puts its own on the CLS rows)."""

    def __init__(self, config=None):
        super().__init__()
        self.config = config or DebertaConfig()
        c = self.config
        if c.hidden_size % c.num_attention_heads or c.hidden_size // c.num_attention_heads != 64:
            raise ValueError("the HIP attention kernels take 64-dim heads (hidden %d / %d heads)"
                             % (c.hidden_size, c.num_attention_heads))
        self.embeddings = DebertaEmbeddings(c)
        self.encoder = DebertaEncoder(c)
        self._init_weights()
        from .encoders import _DropoutStream
        self._rng = _DropoutStream()

    def _init_weights(self):
        """DebertaPreTrainedModel._init_weights: normal(0, 0.02) weights, zero biases (q_bias and v_bias
        included), the padding row zero, LayerNorm (1, 0)."""
        r = self.config.initializer_range
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    m.weight.normal_(0.0, r)
                    if m.bias is not None:
                        m.bias.zero_()
                elif isinstance(m, nn.Embedding):
                    m.weight.normal_(0.0, r)
                    if m.padding_idx is not None:
                        m.weight[m.padding_idx].zero_()
                elif isinstance(m, nn.LayerNorm):
                    m.weight.fill_(1.0)
                    m.bias.zero_()
                elif isinstance(m, DisentangledSelfAttention):
                    m.q_bias.zero_()
                    m.v_bias.zero_()

    def flat_params(self):
        e = self.embeddings
        ps = [e.word_embeddings.weight, e.LayerNorm.weight, e.LayerNorm.bias]
        for l in self.encoder.layer:
            a = l.attention
            ps += [a.self.q_bias, a.self.v_bias, a.self.in_proj.weight, a.self.pos_proj.weight,
                   a.self.pos_q_proj.weight, a.self.pos_q_proj.bias, a.output.dense.weight, a.output.dense.bias,
                   a.output.LayerNorm.weight, a.output.LayerNorm.bias, l.intermediate.dense.weight,
                   l.intermediate.dense.bias, l.output.dense.weight, l.output.dense.bias,
                   l.output.LayerNorm.weight, l.output.LayerNorm.bias]
        ps.append(self.encoder.rel_embeddings.weight)
        return ps

    def drop_site_sizes(self, shapes):
        """Counter counts of the 1 + 4 x layers dropout sites for segments of ``shapes`` = [(nseq, L), ...]
        (the module docstring's layout)."""
        c = self.config
        H, heads = c.hidden_size, c.num_attention_heads
        T = sum(n * l for n, l in shapes)
        rel = sum(2 * l * H for _, l in shapes)
        att = sum(n * heads * l * l for n, l in shapes)
        return [T * H] + [rel, att, T * H, T * H] * c.num_hidden_layers

    def _drop_sites(self, segs, device):
        c = self.config
        if not self.training or (c.hidden_dropout_prob <= 0 and c.attention_probs_dropout_prob <= 0):
            return None
        sizes = self.drop_site_sizes([(s.nseq, s.L) for s in segs])
        seed, off, snap = self._rng.take(sum(sizes), device)
        sites, rel = [], 0
        for n in sizes:
            sites.append(rel)
            rel += n
        return seed, off, snap, sites

    def encode_segments(self, segments):
        """[(input_ids [n, L], attention_mask [n, L]), ...] -> [DebertaOutput per segment] from ONE fused pass."""
        dev = self.embeddings.word_embeddings.weight.device
        c = self.config
        for ids, _ in segments:
            if not 1 <= ids.shape[-1] <= min(DEB_MAX_L, c.max_position_embeddings):
                raise ValueError("the DeBERTa tower takes titles of 1 .. %d tokens (got %d)"
                                 % (min(DEB_MAX_L, c.max_position_embeddings), ids.shape[-1]))
        segs = []
        for ids, mask in segments:
            L.require_gpu(ids.to(dev))
            segs.append(_Segment(ids.to(dev), mask.to(dev)))
        hid = DebertaFn.apply(self.config, segs, self._drop_sites(segs, dev), *self.flat_params())
        outs, r = [], 0
        for s in segs:
            n = s.nseq * s.L
            outs.append(DebertaOutput(hid[r:r + n].view(s.nseq, s.L, -1)))
            r += n
        return outs

    def forward(self, input_ids, attention_mask=None):
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        return self.encode_segments([(input_ids, attention_mask)])[0]


class ClsGeluPoolFn(torch.autograd.Function):
    """PLM's DeBERTa pooler (PLM.py:19-28) on the CLS rows of last_hidden [n, L, H]: gelu(h[:, 0] Wᵀ + b) as one
    gather-operand GEMM with the GELU epilogue (the pre-activation kept for the backward)."""

    @staticmethod
    def forward(ctx, hid, w, b):
        ctx.prec = K.get_gemm_precision()
        n, l, H = hid.shape
        flat = hid.reshape(n * l, H)
        if flat.stride(0) % 4 or flat.stride(1) != 1 or flat.data_ptr() % 16:
            flat = flat.contiguous()
        cls_idx = torch.arange(n, device=hid.device, dtype=torch.int64) * l
        U = _empty(n, H, hid)
        out = _empty(n, H, hid)
        K.gemm(n, H, H, K.operand(flat, L.KCONTIG, rows=cls_idx, mapping=L.ROWS_GATHER), K.operand(w, L.KCONTIG), out,
               bias=b, epilogue=L.EPI_STORE_GELU, c_rows=K.operand(U, L.KCONTIG))
        ctx.save_for_backward(flat, w, cls_idx, U)
        ctx.shape = (n, l, H)
        return out

    @staticmethod
    @_gemm_backward
    def backward(ctx, dout):
        flat, w, cls_idx, U = ctx.saved_tensors
        n, l, H = ctx.shape
        dev = flat.device
        dout = dout.contiguous()
        # dU = dout * gelu'(U): the GELU-gradient epilogue over an identity product
        dU = _empty(n, H, flat)
        K.gemm(n, H, H, K.operand(dout, L.KCONTIG), K.operand(torch.eye(H, device=dev), L.KCONTIG), dU,
               epilogue=L.EPI_GELU_GRAD, c_rows=K.operand(U, L.KCONTIG))
        dw, db = _zeros_views(dev, tuple(w.shape), (H,))
        _proj_wgrad(dU, K.operand(flat, L.MNCONTIG, rows=cls_idx, mapping=L.ROWS_GATHER), dw, db, n)
        dflat = torch.zeros(n * l, H, device=dev)
        K.gemm(n, H, H, K.operand(dU, L.KCONTIG), K.operand(w, L.MNCONTIG), dflat, epilogue=L.EPI_SCATTER,
               c_rows=K.rows_map(cls_idx, L.ROWS_GATHER), pad_row=-1)
        return dflat.view(n, l, H), dw, db
