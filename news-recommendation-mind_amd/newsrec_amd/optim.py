"""Adam on the HIP ``nr_adam`` kernel — a drop-in for the ``torch.optim.Adam`` that
utils/Manager.py:404-413 builds (two param groups, default betas/eps, no weight decay)."""
import weakref

import torch

from . import kernels as K


class FusedAdam(torch.optim.Optimizer):
    """``capturable=True`` keeps each parameter's step count on the device (one multi-tensor
    add per step, bias corrections formed in the kernel), so ``step()`` can be captured in a
    graph and replayed — torch.optim.Adam(capturable=True) semantics.

    ``max_grad_norm``: clip the global gradient norm (over every parameter of the step, both param
    groups, after ``grad_scale``) as ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` would
    before the step (the reference's commented-out utils/Manager.py:646) -- but inside the
    optimizer: one deterministic norm pass (nr_grad_norm_multi) leaves the clip factor on the device
    and the Adam kernel multiplies each gradient by it as it reads it.  ``step()`` NEVER WRITES A
    GRADIENT: unlike torch's in-place clip, ``.grad`` holds the unclipped values afterwards (and the
    row-sparse table flags, which an in-place rewrite would invalidate, stay valid).  No host sync;
    graph-capturable.

    ``skip_nonfinite``: a step whose norm is inf or NaN is dropped -- parameters, moments and step
    counts keep their values -- instead of poisoning them (``max_grad_norm=None`` then means "norm
    and guard only").  Capturable mode decides on the device; otherwise ``step()`` reads the flag
    (ONE host sync per step) before it advances the host step counts.

    ``grad_norm`` (a 0-dim device tensor, no sync) and ``clip_stats()`` (syncs) report the last step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.capturable = capturable
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError("max_grad_norm must be None or a non-negative number")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip = None   # the device nr_clip_state (4 words), created by the first clipped step
        # capturable: each group's lr lives on the device too (read by the kernel), so a graph
        # replay follows group["lr"] changes (a warmup scheduler, Manager.py:415-420) once
        # sync_lr() has copied them over -- step() does it when not capturing, GraphedStep before
        # every replay
        self._lr_dev, self._lr_host = {}, {}

    def sync_lr(self):
        """Copy every group's host lr into its device scalar (only the ones that changed)."""
        for i, group in enumerate(self.param_groups):
            t = self._lr_dev.get(i)
            if t is None:
                dev = next((p.device for p in group["params"]), None)
                if dev is None:
                    continue
                t = self._lr_dev[i] = torch.empty((), dtype=torch.float32, device=dev)
                self._lr_host[i] = None
            if self._lr_host[i] != group["lr"]:
                t.fill_(float(group["lr"]))
                self._lr_host[i] = group["lr"]

    @property
    def clipping(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _clip_state(self, dev=None):
        if self._clip is None:
            if dev is None:
                dev = next(p.device for g in self.param_groups for p in g["params"])
            self._clip = K.clip_state(dev)
        return self._clip

    @property
    def grad_norm(self):
        """The last step's global gradient norm (after ``grad_scale``, before clipping): a 0-dim
        float32 device tensor viewing the clip state -- log it without a sync."""
        return self._clip_state().view(torch.float32)[0]

    def clip_stats(self):
        """{"norm", "scale", "nonfinite", "nonfinite_total"} of the clip state as Python numbers
        (synchronises).  nonfinite_total counts the non-finite steps since the optimizer was made."""
        st = self._clip_state()
        f, i = st.view(torch.float32).tolist(), st.tolist()
        return {"norm": f[0], "scale": f[1], "nonfinite": i[2], "nonfinite_total": i[3]}

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """``grad_scale`` multiplies every gradient as it is read (the data-parallel 1/world
        mean of GradSync), saving a separate scaling pass over the gradients."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = []
        if self.capturable and not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                # a table sharded across ranks (dist.GradSync(shard_tables=True)): this rank updates
                # rows [row0, row0 + rows) only, with moments for those rows
                shard = getattr(p, "_nr_shard", None)
                if shard is not None and self.clipping:
                    # the norm of a table sharded across ranks needs a cross-rank sum
                    raise NotImplementedError("FusedAdam: max_grad_norm / skip_nonfinite with rank-sharded "
                                              "tables (_nr_shard) is not supported")
                if shard is not None and shard[1] == 0:
                    continue
                if len(st) == 0:
                    st["step"] = (torch.zeros((), dtype=torch.int64, device=p.device) if self.capturable else 0)
                    like = p if shard is None else p[shard[0]:shard[0] + shard[1]]
                    st["exp_avg"] = torch.zeros_like(like, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(like, memory_format=torch.contiguous_format)
                todo.append((gi, group, p, st))
        # capturable: the device step counts are advanced by the Adam launch itself
        # (nr_adam_multi_step: the bias corrections use count + 1, the last workgroup adds 1)
        # one nr_adam_multi call per (betas, eps, weight_decay) combination: every tensor of the
        # step in a few launches instead of one launch per parameter
        batches = {}
        for gi, group, p, st in todo:
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            key = (tuple(group["betas"]), group["eps"], group["weight_decay"])
            lr = self._lr_dev[gi] if self.capturable else group["lr"]
            shard = getattr(p, "_nr_shard", None)
            if shard is not None:
                r0, n = shard
                batches.setdefault(key, []).append([p.data[r0:r0 + n], g[r0:r0 + n], st["exp_avg"], st["exp_avg_sq"],
                                                    lr, st])
                continue
            ent = [p, g, st["exp_avg"], st["exp_avg_sq"], lr, st]
            # a row-sparse table gradient (functions.LOCAL_ROW_GRAD) carries per-row "touched" flags:
            # the kernel skips reading the rows known to be zero
            # rt = (that buffer, or a weak reference to the .grad tensor they were bound to, flags, its
            # version counter): the flags hold only while p.grad is that tensor, unmodified since
            # (functions._LocalRowGrad, functions._word_row_flags)
            rt = getattr(p, "_nr_row_touched", None)
            if rt is not None:
                if isinstance(rt[0], weakref.ref):
                    ok = rt[0]() is p.grad
                else:
                    ok = p.grad.data_ptr() == rt[0].data_ptr()
                if ok and p.grad._version == rt[2]:
                    ent.append(rt[1])
            batches.setdefault(key, []).append(ent)

        def entries_of(batch):   # with the step counts as they are now
            return [tuple(e[:5]) + (e[5]["step"],) + tuple(e[6:]) for e in batch]

        if self.clipping and todo:
            # ONE norm over every entry of the step (all batches, both groups), then the clipped Adam
            # per batch reading the scale (and the skip flag) from the device state
            state = self._clip_state(todo[0][2].device)
            max_norm = float("inf") if self.max_grad_norm is None else self.max_grad_norm
            K.grad_norm_multi([e for b in batches.values() for e in entries_of(b)], grad_scale, max_norm, state)
            if self.skip_nonfinite and not self.capturable:
                # host step counts: the decision has to be made here, before they advance (one sync)
                if int(state[2].item()) != 0:
                    return loss
        if not self.capturable:
            for _, _, _, st in todo:
                st["step"] += 1
        for (betas, eps, wd), batch in batches.items():
            if self.clipping:
                K.adam_multi_clip(entries_of(batch), betas[0], betas[1], eps, wd, state,
                                  honor_skip=self.skip_nonfinite, advance_steps=self.capturable)
            else:
                K.adam_multi(entries_of(batch), betas[0], betas[1], eps, wd, grad_scale,
                             advance_steps=self.capturable)
        return loss
