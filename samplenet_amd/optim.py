"""Adam, SGD and RMSprop as ONE launch per parameter group (csrc/optimizer.hip: sn_adam_update, sn_sgd_update, sn_rmsprop_update),
constructed in place of the torch classes -- the three choices of registration/main.py:166-171:

    optimizer = samplenet_amd.optim.Adam(learnable_params, lr=1e-3)                       # --optimizer Adam
    optimizer = samplenet_amd.optim.RMSprop(learnable_params, lr=0.001)                   # --optimizer RMSProp
    optimizer = samplenet_amd.optim.SGD(learnable_params, lr=0.001, momentum=0.9)         # --optimizer SGD
    optimizer = samplenet_amd.optim.make_optimizer(args.optimizer, learnable_params)      # any of the three, by that name

The reference trains everything with Adam by default (registration/main.py:167 torch.optim.Adam; classification/train_samplenet.py:194
and reconstruction/src/samplenet_pointnet_ae.py:206 tf.train.AdamOptimizer -- `tf_epsilon=True` selects TensorFlow's placement of
epsilon); classification/train_classifier.py:133's tf.train.MomentumOptimizer is SGD(momentum=) with no dampening and no Nesterov.
The sampler has about 30 small parameter tensors (249,793 floats): torch's update is a train of host-launched multi-tensor
kernels; each of these is a single launch that a captured training step can carry as its last node
(engine.SamplerTrainStep(optimizer=)).

How it is laid out (_OneLaunchOptimizer, shared by the three)
  * parameters and gradients are addressed where they lie, through a device-side chunk table (multi-tensor-apply style, built on
    the host by build_chunk_table): no parameter is moved or re-allocated -- captured graphs and forward plans hold raw pointers
    into them;
  * the per-element state lives in flat fp32 buffers owned by the optimizer (Adam: exp_avg, exp_avg_sq; SGD: momentum_buffer when
    momentum != 0, nothing otherwise; RMSprop: square_avg, and momentum_buffer when momentum > 0); every tensor's segment starts on
    a 16-byte boundary and state[p][name] are views of them (the torch classes' own state_dict formats: snapshots load both ways);
  * what changes while training -- step count, lr, Adam's running powers beta^t -- lives in a 64-byte device block that the kernel
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
_SGD_UNSUPPORTED = ("maximize", "foreach", "differentiable", "fused")
_RMSPROP_UNSUPPORTED = ("centered", "capturable", "foreach", "maximize", "differentiable")


# ---- pure host functions (tests/test_adam_host.py, tests/test_optim_host.py) --------------------------------------------------------
def plan_segments(sizes):
    """Element offset of every tensor's segment in the flat state buffers (each a multiple of 4 elements = 16 bytes) and the
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


def _walk_state_dict(state_dict, name, required, unsupported):
    """The part of reading a torch-format optimizer state dict that no format owes to its optimizer -> one
    (ids, options, [(id, state[id] or None)]) per parameter group."""
    if not isinstance(state_dict, dict) or set(state_dict) - {"state", "param_groups"} or "state" not in state_dict \
            or "param_groups" not in state_dict:
        raise ValueError("expected a dict with 'state' and 'param_groups'")
    state, out, seen = state_dict["state"], [], set()
    for g in state_dict["param_groups"]:
        opts = {k: v for k, v in g.items() if k != "params"}
        for k in required:
            if k not in opts:
                raise ValueError("param_groups entry without %r" % k)
        for k in unsupported:
            if opts.get(k):
                raise ValueError("samplenet_amd.optim.%s does not implement %s" % (name, k))
        seen.update(g["params"])
        out.append((list(g["params"]), opts, [(i, state.get(i) or None) for i in g["params"]]))
    if set(state) - seen:
        raise ValueError("state for parameters that no group names: %s" % sorted(set(state) - seen))
    return out


def _step_of(i, st):
    t = float(st["step"])
    if t < 0 or t != int(t):
        raise ValueError("state[%r]['step'] = %r is no step count" % (i, t))
    return int(t)


def _one_step(steps):
    if len(steps) > 1:
        raise ValueError("one step count per parameter group: this group holds %s" % sorted(steps))
    return steps.pop() if steps else 0


def parse_state_dict(state_dict):
    """Reads a state dict in torch.optim.Adam's format -- written by torch.optim.Adam or by this class -- without touching a device.
    -> one dict per parameter group: {'ids': [...], 'step': int, 'moments': {id: (exp_avg, exp_avg_sq)}, 'options': {...}}.
    Raises ValueError for what this optimizer cannot represent (amsgrad state, a flag it does not implement, step counts that differ
    inside a group)."""
    out = []
    for ids, opts, entries in _walk_state_dict(state_dict, "Adam", ("lr", "betas", "eps", "weight_decay"), _UNSUPPORTED):
        steps, moments = set(), {}
        for i, st in entries:
            if not st:  # (torch creates a parameter's state at its first gradient)
                continue
            if set(st) != _STATE_KEYS:
                raise ValueError("state[%r] has keys %s, expected %s" % (i, sorted(st), sorted(_STATE_KEYS)))
            steps.add(_step_of(i, st))
            moments[i] = (st["exp_avg"], st["exp_avg_sq"])
        out.append({"ids": ids, "step": _one_step(steps), "moments": moments, "options": opts})
    return out


def parse_sgd_state_dict(state_dict):
    """The same for torch.optim.SGD's format.  -> one dict per parameter group: {'ids', 'step': 1 when any momentum buffer is present
    else 0, 'buffers': {id: momentum_buffer}, 'options'}.  A parameter without state, or whose momentum_buffer is None (torch before
    the parameter's first gradient), has no entry in 'buffers'.  ValueError: a flag not implemented, another state key, buffers
    although momentum == 0, and a group with some buffers present and some missing while dampening != 0 (the kernel keeps ONE
    "first step" flag per group; with dampening == 0 a zeroed buffer and a missing one give the same bits)."""
    out = []
    for ids, opts, entries in _walk_state_dict(state_dict, "SGD", ("lr", "momentum", "dampening", "weight_decay", "nesterov"),
                                               _SGD_UNSUPPORTED):
        buffers = {}
        for i, st in entries:
            if not st:
                continue
            if set(st) != {"momentum_buffer"}:
                raise ValueError("state[%r] has keys %s, expected ['momentum_buffer']" % (i, sorted(st)))
            if st["momentum_buffer"] is not None:
                buffers[i] = st["momentum_buffer"]
        if buffers and opts["momentum"] == 0:
            raise ValueError("momentum buffers in a group with momentum == 0")
        if buffers and len(buffers) < len(ids) and opts["dampening"] != 0:
            raise ValueError("a group with dampening != 0 in which some parameters have a momentum buffer and some have none: "
                             "the first-step rule is kept once per group")
        out.append({"ids": ids, "step": 1 if buffers else 0, "buffers": buffers, "options": opts})
    return out


def parse_rmsprop_state_dict(state_dict):
    """The same for torch.optim.RMSprop's format.  -> one dict per parameter group: {'ids', 'step', 'state': {id: (square_avg,
    momentum_buffer or None)}, 'options'}.  ValueError: centered (its options flag, or a grad_avg in the state), another flag not
    implemented, a key set other than step, square_avg (and momentum_buffer exactly when momentum > 0), step counts that differ
    inside a group."""
    out = []
    for ids, opts, entries in _walk_state_dict(state_dict, "RMSprop", ("lr", "alpha", "eps", "weight_decay", "momentum"),
                                               _RMSPROP_UNSUPPORTED):
        keys = {"step", "square_avg"} | ({"momentum_buffer"} if opts["momentum"] > 0 else set())
        steps, per = set(), {}
        for i, st in entries:
            if not st:
                continue
            if set(st) != keys:
                raise ValueError("state[%r] has keys %s, expected %s" % (i, sorted(st), sorted(keys)))
            steps.add(_step_of(i, st))
            per[i] = (st["square_avg"], st.get("momentum_buffer"))
        out.append({"ids": ids, "step": _one_step(steps), "state": per, "options": opts})
    return out


# ---- the optimizers -----------------------------------------------------------------------------------------------------------------
class _Group:
    """Device side of one parameter group: chunk table, state block and the flat state buffers `names` (attributes of those names)."""

    def __init__(self, opt, group):
        name = opt._NAME
        self.opt = opt
        self.params = [p for p in group["params"] if p.numel() > 0]
        for p in self.params:
            if p.device.type != "cuda":
                raise RuntimeError("%s runs on the GPU only (no CPU fallback): parameter on %s" % (name, p.device))
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError("%s: parameters must be dense contiguous float32 tensors" % name)
        if len({p.device for p in self.params}) > 1:
            raise ValueError("%s: the parameters of a group must live on one device" % name)
        self.device = self.params[0].device if self.params else None
        self.sizes = [p.numel() for p in self.params]
        self.offsets, self.total = plan_segments(self.sizes)
        self.grad_key = None   # the gradient addresses the device table was built from
        self.updated = []      # the parameters that table updates
        self.lr = None         # what word 0 of the device block holds
        self.nchunks = sum((n + CHUNK - 1) // CHUNK for n in self.sizes)
        self.names = ()
        if not self.params:
            return
        self.set_buffers(group)
        self.block = torch.zeros(_STATE_WORDS, dtype=torch.float64, device=self.device)
        self.table = torch.zeros(self.nchunks * _ENTRY.size, dtype=torch.uint8, device=self.device)
        self.write_block(group, 0)
        self.install_views(opt)

    def set_buffers(self, group):
        """Allocates the flat buffers the group's options ask for and drops the others (construction; load_state_dict, where a
        loaded momentum may differ from the constructor's in being zero)."""
        names = self.opt._buffer_names(group)
        for n in names:
            if n not in self.names:
                setattr(self, n, self.opt._alloc(self.total, self.device))
        for n in self.names:
            if n not in names:
                delattr(self, n)
        self.names = names

    def buffer(self, name):
        return getattr(self, name) if name in self.names else None

    def views(self, i):
        o, n, p = self.offsets[i], self.sizes[i], self.params[i]
        return tuple(getattr(self, b)[o:o + n].view_as(p) for b in self.names)

    def install_views(self, opt, step=0):
        for i, p in enumerate(self.params):
            opt.state[p] = opt._state_entry(dict(zip(self.names, self.views(i))), step)

    def write_block(self, group, t):
        """The whole device block for step count t (construction, load_state_dict); stream-ordered."""
        host = torch.zeros(_STATE_WORDS, dtype=torch.float64)
        host[_LR] = float(group["lr"])
        self.opt._block_words(group, t, host)
        host.view(torch.int64)[_T] = t
        self.block.copy_(host)
        self.lr = float(group["lr"])

    def step_count(self):
        return int(self.block.view(torch.int64)[_T].item())  # synchronises


class _OneLaunchOptimizer(torch.optim.Optimizer):
    """What the three updates share: parameter checks, the chunk table and its upload, the device block's lr and t words, prepare() /
    _launch() / _mark_updated() -- the interface engine.SamplerTrainStep(optimizer=) drives -- and the exchange of state dicts.
    A subclass names its flat buffers (_buffer_names), its state entries (_state_entry), its launch (_launch_group) and its state-dict
    reader (_parse, _load_group)."""

    _NAME = "samplenet_amd.optim._OneLaunchOptimizer"
    _UNSUPPORTED = ()
    _GROUP_DEFAULTS = {}   # keys a group written by the torch class lacks

    def __init__(self, params, defaults, given):
        for k in self._UNSUPPORTED:
            if given[k]:
                raise ValueError("%s does not implement %s" % (self._NAME, k))
        if isinstance(defaults["lr"], torch.Tensor):
            raise ValueError("%s: lr must be a number (it is kept on the device by the optimizer itself)" % self._NAME)
        self._dev = []
        super().__init__(params, defaults)

    # -- what a subclass provides ---------------------------------------------------------------------------------------------------
    def _check_options(self, group):
        lr = group["lr"]
        if isinstance(lr, torch.Tensor) or not lr >= 0.0:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not group["weight_decay"] >= 0.0:
            raise ValueError("Invalid weight_decay value: %r" % (group["weight_decay"],))
        for k in self._UNSUPPORTED:
            if group.get(k):
                raise ValueError("%s does not implement %s" % (self._NAME, k))

    def _buffer_names(self, group):
        raise NotImplementedError

    def _state_entry(self, views, step):
        raise NotImplementedError

    def _block_words(self, group, t, host):
        """Words of the device block beyond lr and t (host: the fp64 staging copy)."""

    def _launch_group(self, group, dev):
        raise NotImplementedError

    def _parse(self, state_dict):
        raise NotImplementedError

    def _load_group(self, group, dev, saved):
        """Copies the loaded state of one group (self.state, already on the device) into the flat buffers -> its step count."""
        raise NotImplementedError

    # -- construction ---------------------------------------------------------------------------------------------------------------
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
        for group in self.param_groups:  # (groups written by the torch class lack these)
            for k, v in self._GROUP_DEFAULTS.items():
                group.setdefault(k, v)

    # -- the step -------------------------------------------------------------------------------------------------------------------
    def _sync_lr(self):
        """param_groups[i]['lr'] -> the device block, where it changed (schedulers); a stream-ordered write, no synchronisation."""
        for group, dev in zip(self.param_groups, self._dev):
            lr = float(group["lr"])
            if dev.params and lr != dev.lr:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("%s: lr changed under stream capture; call prepare() before capturing" % self._NAME)
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
                raise RuntimeError("%s: gradients moved under stream capture; call prepare() before capturing" % self._NAME)
            for p in dev.params:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                    raise ValueError("%s: gradients must be dense contiguous float32 tensors on the parameter's device" % self._NAME)
            table = build_chunk_table([p.data_ptr() for p in dev.params], key, dev.sizes)
            assert len(table) == dev.nchunks
            dev.table.copy_(torch.frombuffer(bytearray(pack_chunk_table(table)), dtype=torch.uint8))
            dev.grad_key = key
            dev.updated = [p for p, g in zip(dev.params, key) if g]
        self._sync_lr()

    def _launch(self):
        """One update launch per parameter group on the current stream, from the tables as they are."""
        for group, dev in zip(self.param_groups, self._dev):
            if not dev.params or not dev.updated:
                continue  # (nothing has a gradient: as torch, not a step)
            self._launch_group(group, dev)

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
        """The torch class's format.  Reads the step counts back from the device (synchronises: a checkpoint-time operation)."""
        for dev in self._dev:
            if dev.params:
                dev.install_views(self, dev.step_count())
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Accepts what the torch class's state_dict() or this class's wrote: per-element state is copied into the flat buffers
        (zeroed where the dict has none), the device block is rewritten for the stored step count."""
        parsed = self._parse(state_dict)
        if len(parsed) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        super().load_state_dict(state_dict)  # options into param_groups; state cast onto the parameters' device
        for group, dev, saved in zip(self.param_groups, self._dev, parsed):
            self._check_options(group)
            if not dev.params:
                continue
            dev.set_buffers(group)
            t = self._load_group(group, dev, saved)
            dev.write_block(group, t)
            dev.install_views(self, t)

    def _copy_in(self, dev, i, key, view):
        st = self.state.get(dev.params[i])
        src = st.get(key) if st else None
        if src is not None:
            view.copy_(src)
        else:
            view.zero_()


class Adam(_OneLaunchOptimizer):
    """torch.optim.Adam's constructor (params, lr, betas, eps, weight_decay) plus
        tf_epsilon   True: TensorFlow's form p -= lr sqrt(bc2) / bc1 * m / (sqrt(v) + eps) (classification / reconstruction recipes);
                     False: torch's p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
        grad_scale   factor applied to every gradient inside the update (the 1 / world of a SUM all-reduce; 1 when the reducer
                     averages).
    amsgrad, maximize and torch's other switches raise ValueError when set.  step() is one launch per parameter group on the current
    stream and never synchronises; state_dict() reads the step count back and does."""

    _NAME = "samplenet_amd.optim.Adam"
    _UNSUPPORTED = _UNSUPPORTED
    _GROUP_DEFAULTS = {"tf_epsilon": False, "grad_scale": 1.0}

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, tf_epsilon=False,
                 grad_scale=1.0, foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 decoupled_weight_decay=False):
        given = dict(amsgrad=amsgrad, maximize=maximize, foreach=foreach, capturable=capturable, differentiable=differentiable,
                     fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        # (the unsupported switches stay in the groups with their neutral values: a state dict written here then carries every key
        #  torch.optim.Adam's own groups have)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, tf_epsilon=bool(tf_epsilon), grad_scale=grad_scale,
                        amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=False)
        super().__init__(params, defaults, given)

    def _check_options(self, group):
        super()._check_options(group)
        (b1, b2), eps = group["betas"], group["eps"]
        if not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid betas: %r" % ((b1, b2),))
        if not eps >= 0.0:
            raise ValueError("Invalid epsilon value: %r" % (eps,))

    def _buffer_names(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _state_entry(self, views, step):
        return {"step": torch.tensor(float(step), dtype=torch.float32), **views}

    def _block_words(self, group, t, host):
        b1, b2 = group["betas"]
        host[_B1POW], host[_B2POW] = float(b1) ** t, float(b2) ** t  # (an underflow to 0 is exact enough)

    def _launch_group(self, group, dev):
        b1, b2 = group["betas"]
        check(lib.sn_adam_update(dev.nchunks, ptr(dev.table), ptr(dev.exp_avg), ptr(dev.exp_avg_sq), ptr(dev.block), float(b1),
                                 float(b2), float(group["eps"]), float(group["weight_decay"]), float(group["grad_scale"]),
                                 int(bool(group["tf_epsilon"])), stream_of(dev.block)), "sn_adam_update")

    _parse = staticmethod(parse_state_dict)

    def _load_group(self, group, dev, saved):
        for i in range(len(dev.params)):
            m, v = dev.views(i)
            self._copy_in(dev, i, "exp_avg", m)
            self._copy_in(dev, i, "exp_avg_sq", v)
        return saved["step"]


class SGD(_OneLaunchOptimizer):
    """torch.optim.SGD's constructor (params, lr, momentum, dampening, weight_decay, nesterov) plus grad_scale (see Adam).  maximize,
    foreach, differentiable and fused raise ValueError when set.  With momentum != 0 the group owns one flat momentum_buffer and
    state[p]['momentum_buffer'] are views of it; with momentum == 0 nothing is allocated.

    torch's first momentum step clones the gradient into a buffer that did not exist and applies dampening from the second step on.
    Here "no buffer yet" is the group's step count being zero: ONE flag per parameter group, as Adam's step count is.  It differs
    from torch only for a parameter whose gradient was None in the group's first step, and only when dampening != 0 (with
    dampening == 0 a zeroed buffer and a missing one give the same bits: fmaf(mu, 0, 1 * g1) == g1).

    state_dict() is torch.optim.SGD's format: momentum_buffer is None for every parameter when momentum == 0 or before the first
    step.  load_state_dict() zeroes missing buffers and sets the step count to 1 when any buffer is present, else 0; a group with
    some buffers present and some missing loads only with dampening == 0 (ValueError otherwise, for the reason above)."""

    _NAME = "samplenet_amd.optim.SGD"
    _UNSUPPORTED = _SGD_UNSUPPORTED
    _GROUP_DEFAULTS = {"grad_scale": 1.0, "nesterov": False}

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, grad_scale=1.0, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        given = dict(maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                        grad_scale=grad_scale, maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, given)

    def _check_options(self, group):
        super()._check_options(group)
        mom, damp = group["momentum"], group["dampening"]
        if not mom >= 0.0:
            raise ValueError("Invalid momentum value: %r" % (mom,))
        if not damp >= 0.0:
            raise ValueError("Invalid dampening value: %r" % (damp,))
        if group["nesterov"] and (mom <= 0 or damp != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _buffer_names(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _state_entry(self, views, step):
        return {"momentum_buffer": views.get("momentum_buffer") if step > 0 else None}

    def _launch_group(self, group, dev):
        # (a momentum edited between zero and non-zero after construction no longer matches the buffers: the entry refuses it)
        check(lib.sn_sgd_update(dev.nchunks, ptr(dev.table), ptr(dev.buffer("momentum_buffer")), ptr(dev.block),
                                float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]),
                                float(group["grad_scale"]), int(bool(group["nesterov"])), stream_of(dev.block)), "sn_sgd_update")

    _parse = staticmethod(parse_sgd_state_dict)

    def _load_group(self, group, dev, saved):
        for i in range(len(dev.params)):
            for b in dev.views(i):
                self._copy_in(dev, i, "momentum_buffer", b)
        return saved["step"]


class RMSprop(_OneLaunchOptimizer):
    """torch.optim.RMSprop's constructor (params, lr, alpha, eps, weight_decay, momentum) plus grad_scale (see Adam).  centered=True
    raises ValueError (its sqrt(s - ga^2) cancels: it needs a rounding bound of its own), and so do capturable, foreach, maximize and
    differentiable when set.  State keys are torch's: step, square_avg, and momentum_buffer when momentum > 0; the step count is one
    per parameter group, as Adam's."""

    _NAME = "samplenet_amd.optim.RMSprop"
    _UNSUPPORTED = _RMSPROP_UNSUPPORTED
    _GROUP_DEFAULTS = {"grad_scale": 1.0, "momentum": 0, "centered": False}

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, *, grad_scale=1.0,
                 capturable=False, foreach=None, maximize=False, differentiable=False):
        given = dict(centered=centered, capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable)
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=False, weight_decay=weight_decay,
                        grad_scale=grad_scale, capturable=False, foreach=None, maximize=False, differentiable=False)
        super().__init__(params, defaults, given)

    def _check_options(self, group):
        super()._check_options(group)
        if not group["eps"] >= 0.0:
            raise ValueError("Invalid epsilon value: %r" % (group["eps"],))
        if not group["momentum"] >= 0.0:
            raise ValueError("Invalid momentum value: %r" % (group["momentum"],))
        if not 0.0 <= group["alpha"] < 1.0:
            raise ValueError("Invalid alpha value: %r" % (group["alpha"],))

    def _buffer_names(self, group):
        return ("square_avg", "momentum_buffer") if group["momentum"] > 0 else ("square_avg",)

    def _state_entry(self, views, step):
        return {"step": torch.tensor(float(step), dtype=torch.float32), **views}

    def _launch_group(self, group, dev):
        check(lib.sn_rmsprop_update(dev.nchunks, ptr(dev.table), ptr(dev.square_avg), ptr(dev.buffer("momentum_buffer")),
                                    ptr(dev.block), float(group["alpha"]), float(group["eps"]), float(group["weight_decay"]),
                                    float(group["momentum"]), float(group["grad_scale"]), stream_of(dev.block)), "sn_rmsprop_update")

    _parse = staticmethod(parse_rmsprop_state_dict)

    def _load_group(self, group, dev, saved):
        for i in range(len(dev.params)):
            for key, b in zip(dev.names, dev.views(i)):
                self._copy_in(dev, i, key, b)
        return saved["step"]


def make_optimizer(name, params):
    """The optimizer registration/main.py:166-171 builds for `--optimizer name`: 'Adam' (lr 1e-3), 'RMSProp' (lr 1e-3) or 'SGD'
    (lr 1e-3, momentum 0.9)."""
    if name == "Adam":
        return Adam(params, lr=1e-3)
    if name == "RMSProp":
        return RMSprop(params, lr=0.001)
    if name == "SGD":
        return SGD(params, lr=0.001, momentum=0.9)
    raise ValueError("optimizer %r: one of 'Adam', 'RMSProp', 'SGD'" % (name,))
