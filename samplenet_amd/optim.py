"""Adam as ONE launch per parameter group (csrc/optimizer.hip: sn_adam_update), constructed in place of torch.optim.Adam:

    optimizer = samplenet_amd.optim.Adam(learnable_params, lr=1e-3)          # registration/main.py:167

The reference trains everything with Adam (registration/main.py:167 torch.optim.Adam; classification/train_samplenet.py:194 and
reconstruction/src/samplenet_pointnet_ae.py:206 tf.train.AdamOptimizer -- `tf_epsilon=True` selects TensorFlow's placement of
epsilon).  The sampler has about 30 small parameter tensors (249,793 floats): torch's update is a train of host-launched multi-tensor
kernels; this one is a single launch that a captured training step can carry as its last node (engine.SamplerTrainStep(optimizer=)).

How it is laid out
  * parameters and gradients are addressed where they lie, through a device-side chunk table (multi-tensor-apply style, built on
    the host by build_chunk_table): no parameter is moved or re-allocated -- captured graphs and forward plans hold raw pointers
    into them;
  * the two moments live in two flat fp32 buffers owned by the optimizer; every tensor's segment starts on a 16-byte boundary and
    state[p]['exp_avg'] / ['exp_avg_sq'] are views of them (torch.optim.Adam's own state_dict format: snapshots load both ways);
  * what changes while training -- step count, lr, the running powers beta^t -- lives in a 64-byte device block that the kernel
    advances itself: the launch is the same every step, nothing synchronises with the host.  The step count is ONE per parameter
    group (torch keeps one per parameter: they differ only for a parameter whose gradient was None in some steps).

GPU only, fp32 only: there is no CPU fallback.
"""
import struct

import torch

from ._lib import check, lib, ptr, stream_of

CHUNK = lib.sn_adam_chunk_elems()      # elements one workgroup updates
_ENTRY = struct.Struct("<QQqii")        # csrc/optimizer.hip: SnAdamChunk
_STATE_WORDS = lib.sn_adam_state_bytes() // 8
_LR, _B1POW, _B2POW, _T = 0, 1, 2, 3    # 8-byte words of the device block (SnAdamState)
_UNSUPPORTED = ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay")
_STATE_KEYS = {"step", "exp_avg", "exp_avg_sq"}


# ---- pure host functions (tests/test_adam_host.py) ----------------------------------------------------------------------------------
def plan_segments(sizes):
    """Element offset of every tensor's segment in the flat moment buffers (each a multiple of 4 elements = 16 bytes) and the
    buffers' length.  -> (offsets, total)"""
    offsets, off = [], 0
    for n in sizes:
        if n < 0:
            raise ValueError("negative tensor size")
        offsets.append(off)
        off += (n + 3) // 4 * 4
    return offsets, off


def build_chunk_table(param_ptrs, grad_ptrs, sizes, chunk=None):
    """The chunk table as a list of (param address, gradient address or 0, moment offset, count): tensor by tensor, `chunk`
    elements at a time, never across a tensor boundary.  grad_ptrs[i] None / 0: the tensor's chunks carry a NULL gradient and are
    skipped by the kernel (the table keeps one shape whatever the gradients do)."""
    chunk = CHUNK if chunk is None else chunk
    if chunk <= 0 or chunk % 4:
        raise ValueError("chunk must be a positive multiple of 4")
    offsets, _ = plan_segments(sizes)
    table = []
    for pp, gp, n, off in zip(param_ptrs, grad_ptrs, sizes, offsets):
        if pp % 4 or (gp or 0) % 4:
            raise ValueError("parameter / gradient addresses must be 4-byte aligned")
        for s in range(0, n, chunk):
            table.append((pp + 4 * s, (gp + 4 * s) if gp else 0, off + s, min(chunk, n - s)))
    return table


def pack_chunk_table(table):
    """-> bytes, 32 per entry (the device layout)."""
    return b"".join(_ENTRY.pack(p, g, off, cnt, 0) for p, g, off, cnt in table)


def parse_state_dict(state_dict):
    """Reads a state dict in torch.optim.Adam's format -- written by torch.optim.Adam or by this class -- without touching a device.
    -> one dict per parameter group: {'ids': [...], 'step': int, 'moments': {id: (exp_avg, exp_avg_sq)}, 'options': {...}}.
    Raises ValueError for what this optimizer cannot represent (amsgrad state, a flag it does not implement, step counts that differ
    inside a group)."""
    if not isinstance(state_dict, dict) or set(state_dict) - {"state", "param_groups"} or "state" not in state_dict \
            or "param_groups" not in state_dict:
        raise ValueError("expected a dict with 'state' and 'param_groups'")
    state, out, seen = state_dict["state"], [], set()
    for g in state_dict["param_groups"]:
        opts = {k: v for k, v in g.items() if k != "params"}
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k not in opts:
                raise ValueError("param_groups entry without %r" % k)
        for k in _UNSUPPORTED:
            if opts.get(k):
                raise ValueError("samplenet_amd.optim.Adam does not implement %s" % k)
        steps, moments = set(), {}
        for i in g["params"]:
            seen.add(i)
            st = state.get(i)
            if not st:  # (torch creates a parameter's state at its first gradient)
                continue
            if set(st) != _STATE_KEYS:
                raise ValueError("state[%r] has keys %s, expected %s" % (i, sorted(st), sorted(_STATE_KEYS)))
            t = float(st["step"])
            if t < 0 or t != int(t):
                raise ValueError("state[%r]['step'] = %r is no step count" % (i, t))
            steps.add(int(t))
            moments[i] = (st["exp_avg"], st["exp_avg_sq"])
        if len(steps) > 1:
            raise ValueError("one step count per parameter group: this group holds %s" % sorted(steps))
        out.append({"ids": list(g["params"]), "step": steps.pop() if steps else 0, "moments": moments, "options": opts})
    if set(state) - seen:
        raise ValueError("state for parameters that no group names: %s" % sorted(set(state) - seen))
    return out


# ---- the optimizer ------------------------------------------------------------------------------------------------------------------
class _Group:
    """Device side of one parameter group."""

    def __init__(self, opt, group):
        self.params = [p for p in group["params"] if p.numel() > 0]
        for p in self.params:
            if p.device.type != "cuda":
                raise RuntimeError("samplenet_amd.optim.Adam runs on the GPU only (no CPU fallback): parameter on %s" % p.device)
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError("samplenet_amd.optim.Adam: parameters must be dense contiguous float32 tensors")
        if len({p.device for p in self.params}) > 1:
            raise ValueError("samplenet_amd.optim.Adam: the parameters of a group must live on one device")
        self.device = self.params[0].device if self.params else None
        self.sizes = [p.numel() for p in self.params]
        self.offsets, self.total = plan_segments(self.sizes)
        self.grad_key = None   # the gradient addresses the device table was built from
        self.updated = []      # the parameters that table updates
        self.lr = None         # what word 0 of the device block holds
        self.nchunks = sum((n + CHUNK - 1) // CHUNK for n in self.sizes)
        if not self.params:
            return
        self.exp_avg, self.exp_avg_sq = opt._alloc(self.total, self.device), opt._alloc(self.total, self.device)
        self.block = torch.zeros(_STATE_WORDS, dtype=torch.float64, device=self.device)
        self.table = torch.zeros(self.nchunks * _ENTRY.size, dtype=torch.uint8, device=self.device)
        self.write_block(group, 0)
        self.install_views(opt)

    def views(self, i):
        o, n, p = self.offsets[i], self.sizes[i], self.params[i]
        return self.exp_avg[o:o + n].view_as(p), self.exp_avg_sq[o:o + n].view_as(p)

    def install_views(self, opt, step=0):
        for i, p in enumerate(self.params):
            m, v = self.views(i)
            opt.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}

    def write_block(self, group, t):
        """The whole device block for step count t (construction, load_state_dict); stream-ordered."""
        b1, b2 = group["betas"]
        host = torch.zeros(_STATE_WORDS, dtype=torch.float64)
        host[_LR], host[_B1POW], host[_B2POW] = float(group["lr"]), float(b1) ** t, float(b2) ** t  # (an underflow to 0 is exact enough)
        host.view(torch.int64)[_T] = t
        self.block.copy_(host)
        self.lr = float(group["lr"])

    def step_count(self):
        return int(self.block.view(torch.int64)[_T].item())  # synchronises


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's constructor (params, lr, betas, eps, weight_decay) plus
        tf_epsilon   True: TensorFlow's form p -= lr sqrt(bc2) / bc1 * m / (sqrt(v) + eps) (classification / reconstruction recipes);
                     False: torch's p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
        grad_scale   factor applied to every gradient inside the update (the 1 / world of a SUM all-reduce; 1 when the reducer
                     averages).
    amsgrad, maximize and torch's other switches raise ValueError when set.  step() is one launch per parameter group on the current
    stream and never synchronises; state_dict() reads the step count back and does."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, tf_epsilon=False,
                 grad_scale=1.0, foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 decoupled_weight_decay=False):
        given = dict(amsgrad=amsgrad, maximize=maximize, foreach=foreach, capturable=capturable, differentiable=differentiable,
                     fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        for k in _UNSUPPORTED:
            if given[k]:
                raise ValueError("samplenet_amd.optim.Adam does not implement %s" % k)
        if isinstance(lr, torch.Tensor):
            raise ValueError("samplenet_amd.optim.Adam: lr must be a number (it is kept on the device by the optimizer itself)")
        # (the unsupported switches stay in the groups with their neutral values: a state dict written here then carries every key
        #  torch.optim.Adam's own groups have)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, tf_epsilon=bool(tf_epsilon), grad_scale=grad_scale,
                        amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=False)
        self._dev = []
        super().__init__(params, defaults)

    # -- construction ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_options(group):
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        if isinstance(lr, torch.Tensor) or not lr >= 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid betas: %r" % ((b1, b2),))
        if not eps >= 0.0:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not wd >= 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (wd,))
        for k in _UNSUPPORTED:
            if group.get(k):
                raise ValueError("samplenet_amd.optim.Adam does not implement %s" % k)

    @staticmethod
    def _alloc(n, device):
        """A zeroed flat fp32 buffer of n elements, 16-byte aligned (a hook: the tests put guard words around it)."""
        return torch.zeros(n, dtype=torch.float32, device=device)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_options(group)
            self._dev.append(_Group(self, group))
        except Exception:
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:  # (groups written by torch.optim.Adam carry neither)
            group.setdefault("tf_epsilon", False)
            group.setdefault("grad_scale", 1.0)

    # -- the step -------------------------------------------------------------------------------------------------------------------
    def _sync_lr(self):
        """param_groups[i]['lr'] -> the device block, where it changed (schedulers); a stream-ordered write, no synchronisation."""
        for group, dev in zip(self.param_groups, self._dev):
            lr = float(group["lr"])
            if dev.params and lr != dev.lr:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("samplenet_amd.optim.Adam: lr changed under stream capture; call prepare() before capturing")
                dev.block[_LR:_LR + 1].fill_(lr)
                dev.lr = lr

    def prepare(self):
        """The host side of step(): re-uploads a group's chunk table when a gradient moved or became None (a tuple compare
        otherwise) and writes lr where it changed.  Call it before capturing step() in a graph, and before a replay to make a
        new lr take effect."""
        for dev in self._dev:
            if not dev.params:
                continue
            key = tuple(0 if p.grad is None else p.grad.data_ptr() for p in dev.params)
            if key == dev.grad_key:
                continue
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("samplenet_amd.optim.Adam: gradients moved under stream capture; call prepare() before capturing")
            for p in dev.params:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                    raise ValueError("samplenet_amd.optim.Adam: gradients must be dense contiguous float32 tensors on the parameter's device")
            table = build_chunk_table([p.data_ptr() for p in dev.params], key, dev.sizes)
            assert len(table) == dev.nchunks
            dev.table.copy_(torch.frombuffer(bytearray(pack_chunk_table(table)), dtype=torch.uint8))
            dev.grad_key = key
            dev.updated = [p for p, g in zip(dev.params, key) if g]
        self._sync_lr()

    def _launch(self):
        """One sn_adam_update per parameter group on the current stream, from the tables as they are."""
        for group, dev in zip(self.param_groups, self._dev):
            if not dev.params or not dev.updated:
                continue  # (nothing has a gradient: as torch, not a step)
            b1, b2 = group["betas"]
            check(lib.sn_adam_update(dev.nchunks, ptr(dev.table), ptr(dev.exp_avg), ptr(dev.exp_avg_sq), ptr(dev.block), float(b1),
                                     float(b2), float(group["eps"]), float(group["weight_decay"]), float(group["grad_scale"]),
                                     int(bool(group["tf_epsilon"])), stream_of(dev.block)), "sn_adam_update")

    def _mark_updated(self):
        """The kernel wrote the parameters through raw pointers: bump their autograd version counters, which the package's weight
        caches are keyed on (surface.py, task_features.py, graphed._ModuleGuard)."""
        for dev in self._dev:
            if dev.updated:
                torch.autograd.graph.increment_version(dev.updated)

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.prepare()
        self._launch()
        self._mark_updated()
        return loss

    # -- snapshots ------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.Adam's format.  Reads the step counts back from the device (synchronises: a checkpoint-time operation)."""
        for dev in self._dev:
            if dev.params:
                dev.install_views(self, dev.step_count())
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Accepts what torch.optim.Adam.state_dict() or this class wrote: moments are copied into the flat buffers, the device
        block is rewritten for the stored step count."""
        parsed = parse_state_dict(state_dict)
        if len(parsed) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        super().load_state_dict(state_dict)  # options into param_groups; state cast onto the parameters' device
        for group, dev, saved in zip(self.param_groups, self._dev, parsed):
            self._check_options(group)
            if not dev.params:
                continue
            for i, p in enumerate(dev.params):
                st, (m, v) = self.state.get(p), dev.views(i)
                if st and "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                else:
                    m.zero_()
                    v.zero_()
            dev.write_block(group, saved["step"])
            dev.install_views(self, saved["step"])
