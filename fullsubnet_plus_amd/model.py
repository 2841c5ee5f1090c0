"""FullSubNet+ as a drop-in ``nn.Module`` whose forward runs on libfsnp_hip.so.

Mirrors the reference's plugin surface for the inference path:

* constructor kwargs         speech_enhance/fullsubnet_plus/model/fullsubnet_plus.py:17-34
* parameter tree (strict ``load_state_dict`` of reference checkpoints,
  speech_enhance/audio_zen/inferencer/base_inferencer.py:100-107)
* ``forward(noisy_mag, noisy_real, noisy_imag) -> [B, 2, F, T]``  fullsubnet_plus.py:122-209
* attributes read by callers (``num_groups_in_drop_band``, ``look_ahead``, ...) fullsubnet_plus.py:111-117
* error behaviour: ``AssertionError`` for bad input ranks / channel counts / B == 2
  (fullsubnet_plus.py:136,141; acoustics/feature.py:263), ``NotImplementedError`` for
  unknown options (base_model.py:328, sequence_model.py:72, fullsubnet_plus.py:70).

The modules below only *hold parameters* with the reference's names; no torch op computes
anything in ``forward``.  CPU tensors are rejected: there is deliberately no CPU fallback.
"""
import ctypes
import warnings
import weakref

import torch
import torch.nn as nn

from . import _call, _lib, _policy
from ._args import (_host_lengths, _rate, clipped_pointer, f32_rows, other_rate, output_format, pcm_input, reads_in_place, require_cuda,
                    resample_plan, window_plan_args, window_stream_args)
from ._call import resolve_device as _resolve_device
from ._debug import _DebugHooks

_TCN_DILATIONS = (1, 2, 5, 9, 1, 2, 5, 9)

# Generation counter of the process's module trees: bumped whenever ANY module registers a parameter or a submodule
# (torch's global registration hooks fire for `module.p = nn.Parameter(...)`, load_state_dict(assign=True), add_module,
# replacing a submodule, parametrize).  _HipModel._weights_key re-walks its tree when the counter has moved since it cached its
# parameter list, so a swapped Parameter OBJECT can never leave the handle on the previous checkpoint's weights.
_TREE_GENERATION = [0]


def _bump_tree_generation(*_args, **_kwargs):
    _TREE_GENERATION[0] += 1


nn.modules.module.register_module_parameter_registration_hook(_bump_tree_generation)
nn.modules.module.register_module_module_registration_hook(_bump_tree_generation)


class _StageHolder(nn.Module):
    """A parameter holder that is CALLABLE like the reference's submodule: the call runs the owning model's HIP stage kernels on the branch
    this holder belongs to (_HipModel._attach_holders sets owner, branch and the C entry point).  No torch fallback."""

    def __getstate__(self):              # (the back-reference is re-made by the owner: _HipModel._attach_holders; a weakref does not pickle)
        state = self.__dict__.copy()
        for k in ("_fsnp_owner", "_fsnp_branch", "_fsnp_entry"):
            state.pop(k, None)
        return state

    def _owner(self, otherwise):
        """-> the model whose kernels a call on this holder runs; RuntimeError(otherwise) for a holder that no model attached"""
        owner = self.__dict__.get("_fsnp_owner")
        owner = owner() if owner is not None else None
        if owner is None:
            raise RuntimeError(otherwise)
        return owner

    def forward(self, x):
        owner = self._owner(f"{self.__class__.__name__}: this parameter holder is not a callable stage of a fullsubnet_plus_amd model "
                            "(only the full-band attention layers and TCN stacks of FullSubNet_Plus, and the sub-band recurrent model, are)")
        return owner._stage_call(self.__dict__["_fsnp_entry"], self.__dict__["_fsnp_branch"], x)


class _TSSEParams(_StageHolder):
    """Parameter holder named like ChannelTimeSenseSELayer (attention_model.py:49-76)."""

    def __init__(self, num_channels, kersize, reduction_ratio=2):
        super().__init__()
        reduced = num_channels // reduction_ratio
        for name, k in zip(("smallConv1d", "middleConv1d", "largeConv1d"), kersize):
            setattr(self, name, nn.Sequential(nn.Conv1d(num_channels, num_channels, k, groups=num_channels)))
        self.feature_concate_fc = nn.Linear(3, 1)
        self.fc1 = nn.Linear(num_channels, reduced)
        self.fc2 = nn.Linear(reduced, num_channels)


class _SEParams(_StageHolder):
    """Parameter holder named like ChannelSELayer / ChannelCBAMLayer (attention_model.py:12-23, 302-313)."""

    def __init__(self, num_channels, reduction_ratio=2):
        super().__init__()
        self.fc1 = nn.Linear(num_channels, num_channels // reduction_ratio)
        self.fc2 = nn.Linear(num_channels // reduction_ratio, num_channels)


class _ECAParams(_StageHolder):
    """Parameter holder named like ChannelECAlayer (attention_model.py:343-347)."""

    def __init__(self, k_size=3):
        super().__init__()
        self.conv = nn.Conv1d(1, 1, kernel_size=k_size, padding=(k_size - 1) // 2, bias=False)


class _TCNBlockParams(nn.Module):
    """Parameter holder named like TCNBlock (causal_conv.py:68-94)."""

    def __init__(self, channels, hidden, kernel_size=3):
        super().__init__()
        self.conv1x1 = nn.Conv1d(channels, hidden, 1)
        self.prelu1 = nn.PReLU()
        self.norm1 = nn.GroupNorm(1, hidden, eps=1e-8)
        self.depthwise_conv = nn.Conv1d(hidden, hidden, kernel_size, groups=hidden)
        self.prelu2 = nn.PReLU()
        self.norm2 = nn.GroupNorm(1, hidden, eps=1e-8)
        self.sconv = nn.Conv1d(hidden, channels, 1)


class _FullBandParams(_StageHolder):
    """Parameter holder named like SequenceModel(sequence_model="TCN") (sequence_model.py:47-58,80-81)."""

    def __init__(self, num_freqs, hidden, output_size=None):
        super().__init__()
        self.sequence_model = nn.Sequential(*[_TCNBlockParams(num_freqs, hidden) for _ in _TCN_DILATIONS])
        self.fc_output_layer = nn.Linear(num_freqs, num_freqs if output_size is None else output_size)


class _SubBandParams(_StageHolder):
    """Parameter holder named like SequenceModel(sequence_model="LSTM") (sequence_model.py:31-38,78-79)."""

    def __init__(self, input_size, hidden, output_size, kind="LSTM"):
        super().__init__()
        rnn = nn.LSTM if kind == "LSTM" else nn.GRU                      # sequence_model.py:31-46
        self.sequence_model = rnn(input_size, hidden, num_layers=2, batch_first=True)
        self.fc_output_layer = nn.Linear(hidden, output_size)

    def forward(self, x):
        """SequenceModel.forward (sequence_model.py:97-123) of the sub-band model as a call on the submodule, like the reference's
        `self.sb_model(sb_input)` (fullsubnet_plus.py:203): x [N, input, T] -> [N, output, T] on the fused HIP kernels of the model that
        owns this holder (fsnp_lstm2_fc).  No torch fallback: CPU tensors are refused like forward() refuses them."""
        assert x.dim() == 3, f"The shape of input is {x.shape}."          # sequence_model.py:103
        owner = self._owner("this sub-band model holder is not attached to a fullsubnet_plus_amd model")
        require_cuda(x)
        return owner.lstm2_fc(x)


class _HipState:
    """Owns the fsnp_handle (plain object: its finaliser must not go through nn.Module.__setattr__)."""

    def __init__(self):
        self.handle = None
        self.device = None
        self.packed_key = None

    def close(self):
        h, self.handle, self.device, self.packed_key = self.handle, None, None, None
        if h is not None:
            try:
                _lib.load().fsnp_destroy(h)
            except Exception:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # a copied / pickled module gets its own handle lazily
    def __deepcopy__(self, memo):
        return _HipState()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()


def _reference_style_init(m):
    """Behaviour of BaseModel.weight_init (base_model.py:332-397) for the module kinds on this path (through `.data`, as there)."""
    if isinstance(m, nn.Conv1d):
        nn.init.normal_(m.weight.data)
        if m.bias is not None:
            nn.init.normal_(m.bias.data)
    elif isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight.data)
        nn.init.normal_(m.bias.data)
    elif isinstance(m, (nn.LSTM, nn.GRU)):
        for p in m.parameters():
            (nn.init.orthogonal_ if p.dim() >= 2 else nn.init.normal_)(p.data)


def _check_norm_and_activations(norm_type, *activations):
    """What both constructors refuse like the reference (base_model.py:328, sequence_model.py:96)."""
    if norm_type not in _lib.NORM_TYPES:
        raise NotImplementedError("You must set up a type of Norm. "
                                  "e.g. offline_laplace_norm, cumulative_laplace_norm, forgetting_norm, etc.")
    for act in activations:
        if act and act not in _lib.ACTIVATIONS:
            raise NotImplementedError(f"Not implemented activation function {act}")


class _HipModel(_DebugHooks, nn.Module):
    """Everything the two reference models share on the HIP side: the fsnp_handle, lazy strict weight packing,
    the fsnp_forward call and - from _DebugHooks, the counterpart of include/fsnp_debug.h - the test / bench hooks.
    Subclasses hold the reference's parameter tree and provide ``_config()``."""

    def _attach_holders(self):
        """The sub-band holder is callable like the reference's submodule (`model.sb_model(x)`): it needs to know whose kernels to run."""
        sb = self._modules.get("sb_model")
        if isinstance(sb, _SubBandParams):
            sb.__dict__["_fsnp_owner"] = weakref.ref(self)
        # FullSubNet+: the three attention layers and the three full-band TCN stacks (fullsubnet_plus.py:160-165, 171-173)
        for branch, tag in enumerate(("", "_real", "_imag")):
            for name, entry in (("channel_attention" + tag, "fsnp_channel_attention"), ("fb_model" + tag, "fsnp_fullband_model")):
                mod = self._modules.get(name)
                if isinstance(mod, _StageHolder) and not isinstance(mod, (_SubBandParams, _FullBandLSTMParams)):
                    mod.__dict__.update(_fsnp_owner=weakref.ref(self), _fsnp_branch=branch, _fsnp_entry=entry)

    def __setstate__(self, state):          # copy.deepcopy / pickle: the copy's holder points at the copy
        super().__setstate__(state)
        self._attach_holders()

    def _stage_call(self, entry, branch, x):
        """One of the forward's submodules on a caller's [B, F, T] tensor (fsnp_channel_attention / fsnp_fullband_model)."""
        assert x.dim() == 3, f"The shape of input is {x.shape}."
        require_cuda(x)
        assert x.shape[1] == self.num_freqs, f"expected {self.num_freqs} channels, got {x.shape[1]}"
        lib = self._ensure_handle(x.device)
        x = x if x.dtype == torch.float32 else x.float()
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        st = (ctypes.c_int64 * 3)(*x.stride())
        _call.call(getattr(lib, entry), x.device, self._handle, int(branch), x.data_ptr(), ctypes.byref(st), out.data_ptr(), x.shape[0], x.shape[2])
        return out

    def _init_hip(self):
        # "parity": B > 1 reproduces the reference's drop_band output [B,2,F//2,T] (fullsubnet_plus.py:192-196,
        # fullsubnet.py:107-110); "full": every utterance keeps all bins (== the reference run per utterance).
        self.batch_mode = "parity"
        # What happens to an asynchronous device-side failure (a column-split LSTM launch whose workgroups could not all be
        # resident - a GPU shared with another process - gives up after 2 s and flags the handle):
        #   "sync"     (default) forward() waits for its own launches, polls the flag, and - if it is set - re-runs the
        #              batch once on the one-tile-per-CU kernel (which needs no co-residency) with a warning; a result that
        #              forward() returned is therefore never silently invalid.  The reference's caller synchronises right
        #              after the call anyway (inferencer.py:151-158 moves the mask to the CPU).
        #   "deferred" nothing is waited for (throughput loops, bench.py): call check_errors() / poll_errors() before
        #              trusting results; the next call on the handle also fails loudly.
        self.error_check = "sync"
        # fsnp_watch_weights: every Nth forward starts with one fingerprint kernel over the parameters' storage (1 = every forward)
        self.weight_watch_every = 1
        # how a (re-)pack hands the parameters to the library: "device" = tensors on the handle's device go over as device pointers
        # and the blob is packed by kernels (fsnp_set_weight_device / fsnp_commit_weights_on; raises if a parameter lives elsewhere),
        # "host" = every tensor is copied to the CPU and packed there (fsnp_set_weight / fsnp_commit_weights), "auto" = per tensor
        # whatever its device allows.  The blob is byte-identical either way (profiles/device_weights.md has the timings).
        self.weight_upload = "auto"
        # fsnp_set_verify_sample: every Nth forward of a small batch (a plan of column-split launches only) has one row tile recomputed on
        # an exchange-free kernel beside the following forwards.  None = the policy's default: 16 under error_check="sync", off under
        # "deferred" (throughput loops decide for themselves); an int = that value whatever the policy
        self.verify_sample_every = None
        self._pipeline = False
        self._hip = _HipState()

    # ------------------------------------------------------------------ BaseModel's public helpers (module protocol)
    @staticmethod
    def _stage_input(input):
        assert input.dim() == 4, f"The dim of input is {input.dim()}. It should be four dim."
        require_cuda(input)
        x = input if input.dtype == torch.float32 else input.float()
        return x, (ctypes.c_int64 * 4)(*x.stride())

    @staticmethod
    def unfold(input, num_neighbor):
        """BaseModel.unfold (audio_zen/model/base_model.py:15-47): [B, C, F, T] -> [B, F, C, 2 num_neighbor + 1, T], the overlapped sub-band
        units along the frequency axis (reflect padded); num_neighbor < 1: [B, F, C, 1, T].  HIP kernel (fsnp_unfold) on CUDA tensors of
        any strides.  (The forward never calls it: the recurrent kernels gather the sub-band input on the fly.)"""
        x, st = _HipModel._stage_input(input)
        B, C, F, T = x.shape
        ns = 2 * int(num_neighbor) + 1 if num_neighbor >= 1 else 1
        out = torch.empty((B, F, C, ns, T), dtype=torch.float32, device=x.device)
        _call.call(_lib.load().fsnp_unfold, x.device, x.data_ptr(), ctypes.byref(st), out.data_ptr(), B, C, F, T, int(num_neighbor))
        return out

    def norm_wrapper(self, norm_type: str):
        """BaseModel.norm_wrapper (base_model.py:318-330): -> a callable [B, C, F, T] -> [B, C, F, T] running the named normalisation as HIP
        kernels (fsnp_norm); unknown names raise NotImplementedError like the reference."""
        _check_norm_and_activations(norm_type)
        code = _lib.NORM_TYPES[norm_type]

        def norm(input):
            x, st = _HipModel._stage_input(input)
            B, C, F, T = x.shape
            out = torch.empty((B, C, F, T), dtype=torch.float32, device=x.device)
            _call.call(_lib.load().fsnp_norm, x.device, code, x.data_ptr(), ctypes.byref(st), out.data_ptr(), B, C, F, T)
            return out
        norm.__name__ = norm_type
        return norm

    @property
    def norm(self):
        """`self.norm` of the reference models (fullsubnet_plus.py:115, fullsubnet.py:61): norm_wrapper(self.norm_type)."""
        return self.norm_wrapper(self.norm_type)

    def _weights_key(self):
        # (storage pointer, version) of every parameter: changes on load_state_dict, .to(), in-place updates.  The parameter
        # LIST is cached - walking the module tree (340 parameters) was 0.56 ms per forward, a quarter of a B = 1 step - and
        # rebuilt whenever Parameter OBJECTS may have been replaced: _apply (.to / .float / .cuda ...), and any parameter /
        # submodule registration anywhere in the process since the list was cached (_TREE_GENERATION: assigning a new
        # nn.Parameter to a submodule attribute, load_state_dict(assign=True), replacing a submodule, parametrize).  Deleting
        # a parameter fires no hook: every 256th call re-walks the tree regardless.
        # What NEITHER pointer nor version sees is an edit through `.data` (p.data.add_(), init.normal_(m.weight.data) - the idiom of
        # the reference's own BaseModel.weight_init, base_model.py:339-355 - EMA / weight averaging): `.data` is a fresh tensor
        # with its own version counter on the same storage.  Three nets catch it: (1) on a GPU the handle WATCHES the parameters'
        # storage (fsnp_watch_weights: one fingerprint kernel in front of every forward; forward() re-packs and re-runs under
        # error_check="sync", poll_errors() / check_errors() / the next call say so under "deferred"); (2) the periodic walk folds
        # a content fingerprint into the key (this also covers parameters that cannot be watched: on another device, not fp32);
        # (3) refresh_weights() - what weight_init() calls - forces the re-pack at once.
        cached = self.__dict__.get("_fsnp_plist")
        calls = self.__dict__.get("_fsnp_plist_calls", 0) + 1
        self.__dict__["_fsnp_plist_calls"] = calls
        if cached is None or cached[0] != _TREE_GENERATION[0] or calls % 256 == 0:
            plist = list(self.parameters())
            # (while the handle watches the parameters' storage on the device the fingerprint slot stays None: any change of the
            #  parameter set shows in the pointer tuple, re-packs, and registers the watch again)
            cached = (_TREE_GENERATION[0], plist, None if self.__dict__.get("_fsnp_watched", False) else self._content_fingerprint(plist))
            self.__dict__["_fsnp_plist"] = cached
        return (tuple([(p.data_ptr(), p._version) for p in cached[1]]), cached[2])

    @staticmethod
    def _content_fingerprint(plist):
        """(sum, sum of squares) over all parameter values in fp64: moves with any realistic in-place edit."""
        if not plist:
            return None
        with torch.no_grad():
            by_dev = {}
            for p in plist:
                by_dev.setdefault(p.device, []).append(p.detach().reshape(-1).double())
            s1 = s2 = 0.0
            for ts in by_dev.values():
                flat = torch.cat(ts)
                s1 += float(flat.sum())
                s2 += float((flat * flat).sum())
        return (s1, s2)

    def refresh_weights(self):
        """Force the next forward to re-pack the device weights from the module's parameters.  Call it after editing parameters
        through `.data` (which changes neither a storage pointer nor a version counter): `p.data.add_()`, `init.*_(m.weight.data)`,
        EMA / weight averaging.  On a GPU the handle's weight watch notices such edits by itself (see _weights_key); this is the
        explicit, immediate form - and what weight_init() uses."""
        self._hip.packed_key = None

    def weight_init(self, m):
        """BaseModel.weight_init of the reference (audio_zen/model/base_model.py:332-397), usage `model.apply(model.weight_init)`:
        Conv1d normal / normal, Linear xavier-normal / normal, LSTM / GRU orthogonal matrices and normal biases - through `.data`
        like the reference's, followed by refresh_weights()."""
        _reference_style_init(m)
        self.refresh_weights()

    def _apply(self, fn, *args, **kwargs):
        self.__dict__.pop("_fsnp_plist", None)
        return super()._apply(fn, *args, **kwargs)

    def _ensure_handle(self, device):
        lib = _lib.load()
        st = self._hip
        if st.handle is not None and st.device != device:
            st.close()
        if st.handle is None:
            with torch.cuda.device(device):
                hp = ctypes.c_void_p()
                cfg = self._config()
                _lib.check(lib.fsnp_create(ctypes.byref(cfg), ctypes.byref(hp)), "fsnp_create")
            st.handle, st.device, st.packed_key = hp, device, None
            self.__dict__.pop("_vs_applied", None)
            if self.__dict__.get("_verify_every"):
                _call.check(lib.fsnp_set_verify, hp, int(self.__dict__["_verify_every"]))
            if "_hop_length" in self.__dict__:
                _call.check(lib.fsnp_set_hop_length, hp, self.__dict__["_hop_length"])
        if self._weights_key() != st.packed_key:
            self._upload_weights(lib, device)
            self._watch_parameters(lib, device)
            st.packed_key = self._weights_key()
        return lib

    def _common_config(self):
        """-> an FsnpConfig with the fields both models fill from attributes of the same names; _config() adds the model's own."""
        cfg = _lib.FsnpConfig()
        cfg.num_freqs = self.num_freqs
        cfg.look_ahead = self.look_ahead
        cfg.sb_num_neighbors = self.sb_num_neighbors
        cfg.fb_num_neighbors = self.fb_num_neighbors
        cfg.sb_hidden = self.sb_model_hidden_size
        cfg.output_size = self.output_size
        cfg.norm_type = _lib.NORM_TYPES[self.norm_type]
        cfg.fb_act = _lib.ACTIVATIONS[self.fb_output_activate_function or None]
        cfg.sb_act = _lib.ACTIVATIONS[self.sb_output_activate_function or None]
        cfg.num_groups_in_drop_band = self.num_groups_in_drop_band
        cfg.sequence_model = _lib.SEQUENCE_MODELS[self.sequence_model]
        return cfg

    def _upload_plan(self, device):
        """[(name, tensor, "host" | "device")] over state_dict(): which setter each tensor goes through under self.weight_upload."""
        mode = self.weight_upload
        if mode not in ("auto", "host", "device"):
            raise ValueError(f"weight_upload must be \"auto\", \"host\" or \"device\", got {mode!r}")
        plan = []
        for name, tensor in self.state_dict().items():
            on_dev = mode != "host" and tensor.device == device
            if mode == "device" and not on_dev:
                raise RuntimeError(f"weight_upload=\"device\": {name} is on {tensor.device}, not on {device}")
            plan.append((name, tensor, "device" if on_dev else "host"))
        return plan

    def _upload_weights(self, lib, device):
        """The re-pack under every weight_upload: tensors that _upload_plan marks "device" go to fsnp_set_weight_device on the current
        stream (converted there first if they are not contiguous fp32; the library copies them into its own arena in stream order, so
        a temporary may be released right away), the others ("host": every tensor) to fsnp_set_weight; fsnp_commit_weights_on then
        packs on the device when every tensor came that way, else on the host exactly as fsnp_commit_weights does."""
        h = self._hip.handle

        def upload(stream):                 # (one device context and one stream for the few hundred setter calls of a re-pack)
            for name, tensor, where in self._upload_plan(device):
                if where == "device":
                    t = tensor.detach()
                    if t.dtype != torch.float32 or not t.is_contiguous():
                        t = t.to(torch.float32).contiguous()
                    _lib.check(lib.fsnp_set_weight_device(h, name.encode(), t.data_ptr(), t.numel(), stream), f"fsnp_set_weight_device({name})")
                else:
                    t = tensor.detach().to("cpu", torch.float32).contiguous()
                    _lib.check(lib.fsnp_set_weight(h, name.encode(), t.data_ptr(), t.numel()), f"fsnp_set_weight({name})")
            return lib.fsnp_commit_weights_on(h, stream)
        _call.call(upload, device, what="fsnp_commit_weights_on")

    def _watch_parameters(self, lib, device):
        """fsnp_watch_weights over the parameters' own storage - possible when every parameter is contiguous fp32 on the handle's
        device (what `.to(device)` leaves); otherwise the periodic content fingerprint of _weights_key is the net."""
        plist = self.__dict__["_fsnp_plist"][1]
        ok = bool(plist) and all(p.device == device and p.dtype == torch.float32 and p.is_contiguous() for p in plist)
        n = len(plist) if ok else 0
        ptrs = (ctypes.c_void_p * max(n, 1))(*([p.data_ptr() for p in plist] if ok else [None]))
        nums = (ctypes.c_int64 * max(n, 1))(*([p.numel() for p in plist] if ok else [0]))
        _call.call(lib.fsnp_watch_weights, device, self._hip.handle, ptrs, nums, n, max(1, int(self.weight_watch_every)))
        was = self.__dict__.get("_fsnp_watched", False)
        self.__dict__["_fsnp_watched"] = ok
        if ok != was:                       # the key's fingerprint slot follows (None while the device watches)
            self.__dict__.pop("_fsnp_plist", None)
            self._weights_key()

    @property
    def _handle(self):
        if self._hip.handle is None:
            raise RuntimeError("no HIP handle yet: run a forward on a CUDA tensor first")
        return self._hip.handle

    def _forward_impl(self, ins, batch_offset, global_batch, complex_in=False, lengths=None):
        """ins: 1 (FullSubNet) or 3 (FullSubNet+) tensors [B, 1, F, T], or - complex_in - ONE complex64 [B, F, T]
        tensor (the STFT itself, fsnp_forward_complex); returns the cIRM tensor.  lengths: None, or frames per utterance
        (fsnp_forward_lengths / fsnp_forward_complex_lengths)."""
        noisy_mag = ins[0]
        if complex_in:
            assert noisy_mag.dim() == 3 and noisy_mag.dtype == torch.complex64
            batch_size, num_freqs, num_frames = noisy_mag.size()
        else:
            assert noisy_mag.dim() == 4
            batch_size, num_channels, num_freqs, num_frames = noisy_mag.size()
            assert num_channels == 1, f"{self.__class__.__name__} takes the mag feature as inputs."
        for t in ins[1:]:
            assert t.shape == noisy_mag.shape
        assert num_freqs == self.num_freqs, f"expected {self.num_freqs} frequency bins, got {num_freqs}"
        require_cuda(noisy_mag)
        device = noisy_mag.device
        if lengths is not None:
            if int(batch_offset) != 0 or global_batch is not None:
                raise ValueError("lengths: sharded batches (batch_offset / global_batch) are not supported with per-utterance lengths")
            if batch_size > 1 and self.batch_mode == "parity":
                raise ValueError("lengths: per-utterance lengths need per-utterance semantics; set model.batch_mode = \"full\" "
                                 "(batch_mode \"parity\" mixes the utterances of a batch, feature.py:263)")
            lengths = _host_lengths(lengths, batch_size, f"{self.__class__.__name__}.forward")
        gb = batch_size if global_batch is None else int(global_batch)
        parity = gb > 1 and self.batch_mode == "parity"
        if parity:
            assert gb > self.num_groups_in_drop_band, \
                f"Batch size = {gb}, num_groups = {self.num_groups_in_drop_band}. " \
                f"The batch size should larger than the num_groups."
            parity = self.num_groups_in_drop_band > 1        # drop_band with one group returns its input (feature.py:265)
        if not complex_in:
            ins = [t if t.dtype == torch.float32 else t.float() for t in ins]
        for t in ins:
            assert t.device == device
        lib = self._ensure_handle(device)
        vs = self.verify_sample_every
        vs = (16 if self.error_check == "sync" else 0) if vs is None else int(vs)
        if vs != self.__dict__.get("_vs_applied"):
            if lib.fsnp_set_verify_sample(self._handle, vs) == 0:
                self.__dict__["_vs_applied"] = vs
        out_f = num_freqs // self.num_groups_in_drop_band if parity else num_freqs
        standalone = global_batch is None
        out = torch.empty((gb if parity else batch_size, self.output_size, out_f, num_frames), dtype=torch.float32, device=device)
        if parity and not standalone:
            out.zero_()     # a shard writes only its own rows of the global tensor
        # the entry point without lengths takes the sharding arguments where the one with lengths (never sharded, never parity) has none
        shard = (_lib.MODE_PARITY if parity else _lib.MODE_FULL, int(batch_offset), gb) if lengths is None else ()
        if complex_in:
            fn = lib.fsnp_forward_complex if lengths is None else lib.fsnp_forward_complex_lengths
            strides = (ctypes.c_int64 * 3)(*noisy_mag.stride())
            ptrs = [torch.view_as_real(noisy_mag).data_ptr()]
        else:
            fn = lib.fsnp_forward if lengths is None else lib.fsnp_forward_lengths
            strides = (ctypes.c_int64 * 3 * 3)()
            for i, t in enumerate(ins):
                sb, _, sf, st = t.stride()
                strides[i][0], strides[i][1], strides[i][2] = sb, sf, st
            ptrs = [t.data_ptr() for t in ins] + [None] * (3 - len(ins))
        lens = () if lengths is None else (lengths,)
        args = (self._handle, *ptrs, ctypes.byref(strides), *lens, out.data_ptr(), batch_size, num_frames, *shard)
        _policy.enqueue_retrying_stale(lambda: _call.enqueue(fn, device, *args), self._stale_weights_noticed,
                                       "fsnp_forward_complex" if complex_in else "fsnp_forward")
        return out

    def _stale_weights_noticed(self):
        """The weight watch flagged an EARLIER call (_policy.enqueue_retrying_stale): say so and re-pack."""
        warnings.warn("fullsubnet_plus_amd: parameters were modified in place through .data after they were packed; forwards since "
                      "that edit ran on the OLD weights (error_check='deferred' does not wait for the watch).  Re-packing now; call "
                      "model.refresh_weights() after such edits", RuntimeWarning)
        self._repack()

    def _repack(self):
        self._hip.packed_key = None
        self._ensure_handle(self._hip.device)

    def _wait_and_poll(self):
        """Wait for everything enqueued on the handle's device's current stream -> fsnp_poll_errors' code."""
        if self._pipeline:
            self.flush()
        torch.cuda.current_stream(self._hip.device).synchronize()
        return _lib.load().fsnp_poll_errors(self._handle)

    def _checked(self, run):
        """Runs `run()` (one forward) under the handle's error policy (see error_check in _init_hip, and _policy)."""
        return _policy.run_checked(run, "fsnp_forward", sync=self.error_check == "sync", wait_and_poll=self._wait_and_poll,
                                   repack=self._repack, fallback=self._one_tile_per_cu)

    def _one_tile_per_cu(self, run):
        """_policy.run_checked's fallback after a timed-out or wrongly verified exchange: the batch once more on the kernel without one
        (a model that has no such kernel still defers its column-split chunks when pipelined: _wait_and_poll's flush)."""
        lib = _lib.load()
        warnings.warn(f"fullsubnet_plus_amd: {_lib.last_error()}; re-running this batch on the one-tile-per-CU kernel", RuntimeWarning)
        prev = self.__dict__.get("_lstm_coop_mode", 1)
        _call.check(lib.fsnp_debug_set_lstm_coop, self._handle, 0)
        try:
            out = run()
            _lib.check(self._wait_and_poll(), "fsnp_forward (retry)")
        finally:
            lib.fsnp_debug_set_lstm_coop(self._handle, prev)      # the mode the caller had set (debug_set_lstm_coop), not always 1
        return out

    def set_verify(self, every, device="cuda"):
        """Exchange verification (fsnp_set_verify): every `every`-th forward whose plan holds a column-split launch runs those
        sequences again on the one-tile-per-CU kernel (no inter-workgroup exchange) and compares on the device; a mismatch flags
        the handle (code 7: error_check="sync" then re-runs the batch on the one-tile-per-CU kernel with a RuntimeWarning,
        "deferred" reports through poll_errors() / check_errors() / the next call).  0 = off.  Also `model.verify_every = N`
        before the first forward, or FSNP_VERIFY_EVERY=N in the environment."""
        self.__dict__["_verify_every"] = int(every)
        self._setting("fsnp_set_verify", int(every), device=device)

    @property
    def verify_every(self):
        return self.__dict__.get("_verify_every", 0)

    @verify_every.setter
    def verify_every(self, every):
        self.__dict__["_verify_every"] = int(every)
        if self._hip.handle is not None:
            _call.check(_lib.load().fsnp_set_verify, self._handle, int(every))

    @property
    def hop_length(self):
        """The hop of the waveform path in samples (include/fsnp_stft_geometry.h), what the reference reads from [acoustics] of its TOML
        next to n_fft = win_length = 2 (num_freqs - 1): stft, istft, enhance_wave (with and without lengths=), reserve(max_samples=...)
        and open_wave_stream run at it.  Default num_freqs - 1 (n_fft / 2).  Assigning validates first and touches no GPU: ValueError
        unless n_fft / 8 <= hop_length <= n_fft / 2 and hop_length % 4 == 0.  A wave session keeps the hop it was opened with."""
        return self.__dict__.get("_hop_length", self.num_freqs - 1)

    @hop_length.setter
    def hop_length(self, hop):
        from .stream import hop_refusal
        why = hop_refusal(self.num_freqs, hop)
        if why is not None:
            raise ValueError(f"{self.__class__.__name__}.hop_length: {why}")
        self.__dict__["_hop_length"] = int(hop)
        if self._hip.handle is not None:
            _call.check(_lib.load().fsnp_set_hop_length, self._handle, int(hop))

    @property
    def sample_rate(self):
        """The rate in Hz the model's weights were trained at and its STFT runs at: `sr` of [acoustics] in the reference's TOML, 16000
        unless assigned.  enhance_wave(..., sample_rate=R), resample and reserve(..., sample_rate=R) convert between R and this rate
        (include/fsnp_resample.h).  Held in Python and passed with every call; assigning validates (ValueError unless a positive
        integer) and touches no GPU.  open_wave_stream(..., sample_rate=R) opens a wave session that converts inside every push
        (include/fsnp_wave_rate_stream.h); spectrum and stream sessions see no samples and take no rate."""
        return self.__dict__.get("_sample_rate", 16000)

    @sample_rate.setter
    def sample_rate(self, rate):
        self.__dict__["_sample_rate"] = _rate(rate, f"{self.__class__.__name__}.sample_rate")

    def verify_count(self):
        """-> verification passes run so far (fsnp_verify_count)."""
        return int(_lib.load().fsnp_verify_count(self._handle))

    def poll_errors(self):
        """Raise if a finished launch flagged the handle; no synchronisation (fsnp_poll_errors)."""
        _call.check(_lib.load().fsnp_poll_errors, self._handle)

    def check_errors(self):
        """Synchronise and raise if an earlier call failed on the device (see fsnp_check_errors)."""
        _call.check(_lib.load().fsnp_check_errors, self._handle)

    def set_precision(self, mode, device="cuda"):
        """"fp32" (default) or "bf16_ih" (BASELINE.json configs[4]: layer-1 ih-GEMM of the sub-band LSTM in bf16; fsnp.h)."""
        assert mode in ("fp32", "bf16_ih")
        self._setting("fsnp_set_precision", {"fp32": 0, "bf16_ih": 1}[mode], device=device)

    def set_pipeline(self, enable=True, device="cuda"):
        """Pipelined serving mode (include/fsnp.h: fsnp_set_pipeline): the remainder chunks of the sub-band plan overlap
        the NEXT forward's full-band stages.  Outputs are complete only after flush()."""
        self._setting("fsnp_set_pipeline", int(bool(enable)), device=device)
        self._pipeline = bool(enable)

    def _setting(self, entry, *values, device="cuda"):
        """One of the handle's setters, fsnp_set_* / fsnp_debug_set_*(handle, values...), on the handle of `device` (created if need be)."""
        lib = self._ensure_handle(_resolve_device(device))
        _call.check(getattr(lib, entry), self._handle, *values)

    def reserve(self, max_batch, max_frames, max_samples=0, device="cuda", sample_rate=None):
        """Grow the handle's workspace once to what any forward of <= max_batch utterances x max_frames frames needs (and the
        STFT / iSTFT area of enhance_wave for max_samples samples per utterance): a serving loop with varying clip lengths then
        never re-allocates (fsnp_reserve; stream-ordered on the current stream, no device synchronisation).  sample_rate: the rate
        enhance_wave will be called with; max_samples then counts at that rate, max_frames stays in model steps, and the tap tables
        of both directions are uploaded too (fsnp_reserve_rate)."""
        rate = other_rate(sample_rate, self.sample_rate, f"{self.__class__.__name__}.reserve")
        dev = _resolve_device(device)
        lib = self._ensure_handle(dev)
        mode = _lib.MODE_PARITY if (self.batch_mode == "parity" and max_batch > 1 and self.num_groups_in_drop_band > 1) else _lib.MODE_FULL
        _call.call(lib.fsnp_reserve, dev, self._handle, int(max_batch), int(max_frames), mode, 0 if rate else int(max_samples))
        if rate and int(max_samples) > 0:
            _call.call(lib.fsnp_reserve_rate, dev, self._handle, int(max_batch), int(max_samples), rate, self.sample_rate)

    def flush(self):
        """Order the current stream after every deferred launch of earlier forwards (fsnp_flush)."""
        if self._hip.handle is None:
            return
        _call.call(_lib.load().fsnp_flush, self._hip.device, self._handle)

    def forward_complex(self, noisy_complex, batch_offset=0, global_batch=None, lengths=None):
        """the forward fed with the complex64 STFT itself ([B, F, T], any strides - torch.stft's
        output is consumed in place); mag / real / imag are derived inside the HIP repack kernel instead of by the
        three torch ops of inferencer.py:143-147.  Same result as forward(|X|, X.real, X.imag, lengths=lengths)."""
        return self._checked(lambda: self._forward_impl([noisy_complex], batch_offset, global_batch, complex_in=True, lengths=lengths))

    def enhance(self, noisy_complex, lengths=None):
        """SURVEY.md 8(f-1) + (f-3): model forward + decompress_cIRM + complex multiply, all in HIP - lines 143-157 of
        fullsubnet_plus/inferencer/inferencer.py (`full_band_crm_mask` of fullsubnet/inferencer/inferencer.py for the
        original FullSubNet): noisy_complex [B,F,T] complex64 (torch.stft output, any strides) -> enhanced complex
        [B,F,T] ready for torch.istft.  Always keeps all bins (batch_mode "full").  lengths: frames per utterance (see
        forward); frames past them come out as exactly 0 whatever the input holds there (fsnp_apply_cirm_lengths)."""
        assert noisy_complex.dim() == 3 and noisy_complex.is_complex()
        assert self.output_size == 2, "the cIRM epilogue needs the two mask channels (decompress_cIRM, acoustics/mask.py:60-63)"
        if lengths is not None:
            lengths = _host_lengths(lengths, noisy_complex.shape[0], f"{self.__class__.__name__}.enhance")
        mode, self.batch_mode = self.batch_mode, "full"
        try:
            mask = self.forward_complex(noisy_complex, lengths=lengths)
        finally:
            self.batch_mode = mode
        if self._pipeline:
            self.flush()            # the mask's deferred rows (pipelined mode) are complete on this stream only after a flush
        return self._apply_cirm(mask, noisy_complex, lengths)

    # ------------------------------------------------------------------ STFT / iSTFT in HIP
    def stft(self, wav):
        """audio_zen/acoustics/feature.py:10-31 (torch.stft, n_fft = win_length = 2 (F - 1), hop_length = self.hop_length, hann, center)
        in HIP: wav [B, samples] -> complex64 [B, F, T = 1 + samples // hop_length] with torch.stft's strides.  wav: fp32, or
        torch.int16 full-scale PCM (the spectrum of wav.float() / 32768, bit for bit), rows and samples at any strides - one channel
        of an interleaved buffer is read in place (fsnp_stft_pcm)."""
        assert wav.dim() == 2, "expected [B, samples]"
        require_cuda(wav)
        lib = self._ensure_handle(wav.device)
        B, L = wav.shape
        T = 1 + L // self.hop_length
        spec = torch.empty((B, T, self.num_freqs), dtype=torch.complex64, device=wav.device)
        if reads_in_place(wav):
            wav, fmt, row, step = pcm_input(wav)
            _call.call(lib.fsnp_stft_pcm, wav.device, self._handle, wav.data_ptr(), fmt, row, step, torch.view_as_real(spec).data_ptr(), B, L)
        else:
            wav = f32_rows(wav)
            _call.call(lib.fsnp_stft, wav.device, self._handle, wav.data_ptr(), wav.stride(0), torch.view_as_real(spec).data_ptr(), B, L)
        return spec.permute(0, 2, 1)

    def istft(self, spec, length):
        """feature.py:34-56 (torch.istft(..., length=length), at self.hop_length) in HIP: complex64 [B, F, T] (any strides) -> [B, length]."""
        assert spec.dim() == 3 and spec.dtype == torch.complex64 and spec.shape[1] == self.num_freqs
        require_cuda(spec)
        lib = self._ensure_handle(spec.device)
        B, _, T = spec.shape
        out = torch.empty((B, int(length)), dtype=torch.float32, device=spec.device)
        st = (ctypes.c_int64 * 3)(*spec.stride())
        _call.call(lib.fsnp_istft, spec.device, self._handle, torch.view_as_real(spec).data_ptr(), ctypes.byref(st), out.data_ptr(), out.stride(0),
                   B, T, int(length))
        return out

    def enhance_wave(self, noisy, lengths=None, out_format=None, clipped=None, sample_rate=None):
        """The reference inferencer's inner loop in ONE call (fullsubnet_plus/inferencer/inferencer.py:142-158,
        `mag_complex_full_band_crm_mask`; `full_band_crm_mask` of fullsubnet/inferencer/inferencer.py for the original
        FullSubNet): noisy waveform [B, samples] -> enhanced waveform [B, samples]; STFT, model (all bins), cIRM
        decompression, complex multiply and iSTFT all run in HIP on the caller's stream, the two transforms at self.hop_length
        (1 + samples // hop_length model steps).  lengths: None, or SAMPLES per
        utterance (a Python sequence or a CPU integer tensor): row b is then enhance_wave(noisy[b:b+1, :lengths[b]]) of that
        clip alone, and 0 past lengths[b].  Follows error_check like forward: under "deferred", too, a `.data` edit that the weight
        watch flagged on an earlier call is answered by a RuntimeWarning, a re-pack and the edited weights' result.

        PCM (include/fsnp_pcm.h): noisy may be torch.int16 (full scale: what noisy.float() / 32768 gives, bit for bit) and may have
        any strides - a channel of an interleaved buffer is read in place, nothing is converted or copied in front.  out_format: None
        (follow the input: float -> fp32 as ever, int16 -> "s16"), "f32", "s16" (int16, round half to even, saturating) or "s16_peak"
        (int16, the reference CLI's peak normalisation np.int16(0.8 * 32767 * y / max|y|) over each clip's own samples).  clipped:
        optional int32 CUDA tensor [B], overwritten with the number of samples of each row that saturated or were NaN ("s16" only:
        0 for the other formats).

        sample_rate (include/fsnp_resample.h): None or self.sample_rate is the call as it has always been.  Any other rate in Hz: noisy
        [B, L] holds samples at that rate and so does the result [B, L]; lengths count samples at that rate.  The clip is converted
        to the model's rate inside the kernel that pads it for the STFT and the result is converted back on the way out, by one
        fixed polyphase FIR: the call gives, bit for bit, resample(enhance_wave(resample(noisy, R, M)), M, R)[:, :L] - with lengths,
        row b is that composition of noisy[b:b+1, :lengths[b]] alone, bit for bit: the rows then run one clip at a time (the model is
        not bit-identical between batch sizes), which costs the batch's throughput; pad to one length for one batch.  ValueError
        for a rate that is no positive integer or a ratio with max(up, down) > 640, before any GPU is touched."""
        assert self.output_size == 2, "the cIRM epilogue needs the two mask channels (decompress_cIRM, acoustics/mask.py:60-63)"
        assert noisy.dim() == 2, "expected [B, samples]"
        rate = other_rate(sample_rate, self.sample_rate, f"{self.__class__.__name__}.enhance_wave")
        ofmt, out_dtype = output_format(out_format, noisy.dtype, "enhance_wave")
        require_cuda(noisy)
        samples = None if lengths is None else _host_lengths(lengths, noisy.shape[0], f"{self.__class__.__name__}.enhance_wave")
        B, L = noisy.shape
        if reads_in_place(noisy) or ofmt != _lib.SAMPLE_F32 or clipped is not None or rate is not None:
            # include/fsnp_pcm.h: int16 or floating point at any strides, any output format; fsnp_enhance_wave_rate where the samples'
            # rate is not the model's
            wav, ifmt, row, step = pcm_input(noisy)
            clip = clipped_pointer(clipped, B, wav.device, "enhance_wave")
            fn, rates = ("fsnp_enhance_wave_pcm", ()) if rate is None else ("fsnp_enhance_wave_rate", (rate, self.sample_rate))
            out = torch.empty((B, L), dtype=out_dtype, device=wav.device)
            args = (wav.data_ptr(), ifmt, row, step, out.data_ptr(), ofmt, out.stride(0), 1, samples, B, L, clip, *rates)
        else:
            wav = f32_rows(noisy)
            fn, lens = ("fsnp_enhance_wave", ()) if samples is None else ("fsnp_enhance_wave_lengths", (samples,))
            out = torch.empty((B, L), dtype=torch.float32, device=wav.device)
            args = (wav.data_ptr(), wav.stride(0), out.data_ptr(), out.stride(0), *lens, B, L)
        entry = getattr(self._ensure_handle(wav.device), fn)

        def run():
            _policy.enqueue_retrying_stale(lambda: _call.enqueue(entry, wav.device, self._handle, *args), self._stale_weights_noticed, fn)
            return out
        return self._checked(run)

    def _windowed_call(self, fn, what, noisy, window, overlap, lengths, out_format, clipped, max_batch):
        """Arguments and output of fsnp_enhance_wave_windowed / fsnp_debug_window_roundtrip (include/ext/fsnp_windowed.h, one signature)
        -> (run, out): run() enqueues the call once and returns its code, unchecked."""
        assert noisy.dim() == 2, "expected [B, samples]"
        window, overlap, max_batch = window_plan_args(window, overlap, max_batch, self.num_freqs, what)
        ofmt, out_dtype = output_format(out_format, noisy.dtype, what)
        require_cuda(noisy)
        B, L = noisy.shape
        samples = None if lengths is None else _host_lengths(lengths, B, what)
        wav, ifmt, row, step = pcm_input(noisy)
        clip = clipped_pointer(clipped, B, wav.device, what)
        out = torch.empty((B, L), dtype=out_dtype, device=wav.device)
        entry = getattr(self._ensure_handle(wav.device), fn)
        args = (self._handle, wav.data_ptr(), ifmt, row, step, out.data_ptr(), ofmt, out.stride(0), 1, samples, B, L, window, overlap,
                max_batch, clip)
        return (lambda: _call.enqueue(entry, wav.device, *args)), out

    def enhance_wave_windowed(self, noisy, window, overlap, lengths=None, out_format=None, clipped=None, max_batch=32):
        """One long recording per row: enhance_wave in overlapping windows, cross-faded on the device (include/ext/fsnp_windowed.h,
        DESIGN.md 8f).  noisy [B, samples] -> [B, samples].  window, overlap: samples at the model's rate, with
        n_fft / 2 <= overlap <= window / 2; a clip of L samples is cut into window_count(L, window, overlap) windows that start
        window - overlap samples apart (the last one as long as what is left, more than `overlap`).  Every window is enhanced as a clip
        of its own - its own reflect padding, frames and norms - and where two windows overlap the result fades from the earlier to
        the later one by 0.5 - 0.5 cos(pi j / overlap); at overlap = window / 2 that is the periodic-Hann weighting of the reference's
        Inferencer.overlapped_chunk.  The result is NOT enhance_wave(noisy): there every statistic is taken over the whole recording.

        The windows of all rows run through the model max_batch at a time, across rows.  Windows of one length run as an ordinary
        batch (a call in which no row is longer than `window` and B <= max_batch is enhance_wave, bit for bit); a batch that mixes
        lengths runs like enhance_wave(lengths=) and is refused where that is (subband_num > 1, the sub-band "TCN", a last window too
        short for the TSSE kernels).  noisy, lengths, out_format and clipped follow enhance_wave's rules; there is no sample_rate=
        (compose with resample, INTEGRATION.md "One long recording").  ValueError, before any GPU is touched, for a window or overlap
        that is no integer, an overlap outside its range and max_batch < 1."""
        assert self.output_size == 2, "the cIRM epilogue needs the two mask channels (decompress_cIRM, acoustics/mask.py:60-63)"
        fn = "fsnp_enhance_wave_windowed"
        enqueue, out = self._windowed_call(fn, f"{self.__class__.__name__}.enhance_wave_windowed", noisy, window, overlap, lengths,
                                           out_format, clipped, max_batch)

        def run():
            _policy.enqueue_retrying_stale(enqueue, self._stale_weights_noticed, fn)
            return out
        return self._checked(run)

    def open_window_stream(self, slots, window, overlap, max_samples=4096, max_batch=32, device="cuda"):
        """-> fullsubnet_plus_amd.stream.WindowStream: `slots` independent live audio streams enhanced in the windows of
        enhance_wave_windowed (include/session/fsnp_window_stream.h) - for FullSubNet+, which has no other online form,
        and for the original FullSubNet alike.  Blocks of up to max_samples samples in, as many out, `window` samples late; a
        window runs through the model in the push that completes it, up to max_batch windows of all slots per forward.  All push
        outputs of a clip followed by finish(), without the first `window` samples, are enhance_wave_windowed(clip, window, overlap)
        of that clip alone for any block sizes, bit for bit at max_batch=1 on both sides.  There is no sample_rate= (compose with
        resample).  ValueError, before any GPU is touched, for arguments that are no integers, an overlap outside
        [n_fft / 2, window / 2] and slots, max_samples or max_batch < 1.  What a finish could otherwise refuse is refused here by the
        library (FsnpError, code 2): an overlap so short that a clip's last window may fall below the model's minimum clip (TSSE: 8
        frames, overlap >= 1791 at the default geometry), and subband_num > 1 or the sub-band "TCN" unless max_batch=1."""
        from .stream import WindowStream
        assert self.output_size == 2, "the cIRM epilogue needs the two mask channels (decompress_cIRM, acoustics/mask.py:60-63)"
        args = window_stream_args(slots, window, overlap, max_samples, max_batch, self.num_freqs, f"{self.__class__.__name__}.open_window_stream")
        return WindowStream(self, *args, _resolve_device(device))

    def resample(self, wav, from_rate, to_rate, lengths=None, out_format=None, clipped=None):
        """Sample-rate conversion on the device by the filter enhance_wave(..., sample_rate=) uses (include/fsnp_resample.h; one fixed
        zero-phase polyphase FIR, one thread per output sample): wav [B, L] at from_rate -> [B, ceil(L * up / down)] at to_rate.
        wav, out_format and clipped follow enhance_wave's rules: fp32 or torch.int16 at any strides, read in place; out_format None
        follows the input, or "f32" / "s16" / "s16_peak" (peak over each row's own output samples); clipped an int32 CUDA tensor [B].
        lengths: samples per row at from_rate; row b is then that clip converted alone, 0 from its ceil(lengths[b] * up / down) on.
        from_rate == to_rate is a format-converting copy.  ValueError for a bad rate or ratio before any GPU is touched; a handle
        keeps the tables of 8 (up, down) pairs and refuses a ninth."""
        what = f"{self.__class__.__name__}.resample"
        assert wav.dim() == 2, "expected [B, samples]"
        up, down, _ = resample_plan(from_rate, to_rate, what)
        ofmt, out_dtype = output_format(out_format, wav.dtype, "resample")
        require_cuda(wav)
        samples = None if lengths is None else _host_lengths(lengths, wav.shape[0], what)
        wav, ifmt, row, step = pcm_input(wav)
        B, L = wav.shape
        clip = clipped_pointer(clipped, B, wav.device, "resample")
        lib = self._ensure_handle(wav.device)
        out = torch.empty((B, -(-L * up // down)), dtype=out_dtype, device=wav.device)
        _call.call(lib.fsnp_resample_pcm, wav.device, self._handle, wav.data_ptr(), ifmt, row, step, out.data_ptr(), ofmt, out.stride(0), 1,
                   samples, B, L, int(from_rate), int(to_rate), clip)
        return out

    def _apply_cirm(self, mask, noisy_complex, lengths=None):
        """lengths: None, or the ctypes int32[B] of _host_lengths (frames >= lengths[b] of row b are written as 0)."""
        B, F, T = noisy_complex.shape
        out = torch.empty_strided((B, F, T), noisy_complex.stride(), dtype=torch.complex64, device=noisy_complex.device)
        xr, orr = torch.view_as_real(noisy_complex), torch.view_as_real(out)
        st = (ctypes.c_int64 * 3)(*noisy_complex.stride())
        ost = (ctypes.c_int64 * 3)(*out.stride())
        lib, lens = _lib.load(), () if lengths is None else (lengths,)
        _call.call(lib.fsnp_apply_cirm if lengths is None else lib.fsnp_apply_cirm_lengths, noisy_complex.device,
                   mask.data_ptr(), xr.data_ptr(), ctypes.byref(st), orr.data_ptr(), ctypes.byref(ost), *lens, B, F, T)
        return out

    def lstm2_fc(self, x):
        """Fused sub-band LSTM + Linear alone (sequence_model.py:113-123): x [N, input, T] -> [N, 2, T]."""
        assert x.dim() == 3 and x.is_cuda
        lib = self._ensure_handle(x.device)
        n, _, steps = x.shape
        xt = x.permute(0, 2, 1).contiguous().float()
        out = torch.empty((n, self.output_size, steps), dtype=torch.float32, device=x.device)
        _call.call(lib.fsnp_lstm2_fc, x.device, self._handle, xt.data_ptr(), out.data_ptr(), n, steps)
        return out


class FullSubNet_Plus(_HipModel):
    def __init__(self,
                 num_freqs,
                 look_ahead,
                 sequence_model,
                 fb_num_neighbors,
                 sb_num_neighbors,
                 fb_output_activate_function,
                 sb_output_activate_function,
                 fb_model_hidden_size,
                 sb_model_hidden_size,
                 channel_attention_model="SE",
                 norm_type="offline_laplace_norm",
                 num_groups_in_drop_band=2,
                 output_size=2,
                 subband_num=1,
                 kersize=[3, 5, 10],
                 weight_init=True,
                 ):
        super().__init__()
        assert sequence_model in ("GRU", "LSTM", "TCN"), f"{self.__class__.__name__} only support GRU, LSTM and TCN."
        if sequence_model not in _lib.SEQUENCE_MODELS:
            raise NotImplementedError(f"Not implemented {sequence_model}")                 # sequence_model.py:72
        if channel_attention_model not in _lib.ATTENTION:
            raise NotImplementedError(f"Not implemented channel attention model {channel_attention_model}")
        if subband_num != 1 and channel_attention_model != "ECA":
            # fullsubnet_plus.py:47-50,155-163: the reference builds its TSSE / SE / CBAM layers for
            # num_freqs // subband_num + 1 channels and then feeds the real / imag branches num_freqs channels - its own
            # forward raises; only ECA (no per-channel parameters) runs.
            raise NotImplementedError("subband_num != 1 only works with channel_attention_model='ECA' (as in the reference)")
        if subband_num < 1:
            raise NotImplementedError("subband_num must be >= 1")
        _check_norm_and_activations(norm_type, fb_output_activate_function, sb_output_activate_function)

        self.num_channels = num_freqs
        def make_attention():
            if channel_attention_model == "TSSE":
                return _TSSEParams(num_freqs, kersize)
            if channel_attention_model == "ECA":
                return _ECAParams()
            return _SEParams(num_freqs)                      # SE and CBAM share the parameter tree
        self.channel_attention_model = channel_attention_model
        self.channel_attention = make_attention()
        self.channel_attention_real = make_attention()
        self.channel_attention_imag = make_attention()
        # NB: the reference hard-codes the TCNBlock hidden width to 512 (causal_conv.py:68) and ignores
        # fb_model_hidden_size for the TCN full-band models (sequence_model.py:48-57).
        self.fb_model = _FullBandParams(num_freqs, 512)
        self.fb_model_real = _FullBandParams(num_freqs, 512)
        self.fb_model_imag = _FullBandParams(num_freqs, 512)
        sb_in = (sb_num_neighbors * 2 + 1) + 3 * (fb_num_neighbors * 2 + 1)
        if sequence_model == "TCN":      # sequence_model.py:47-58,80-81: TCNBlocks keep the default 512 hidden channels
            self.sb_model = _FullBandParams(sb_in, 512, output_size)
        else:
            self.sb_model = _SubBandParams(sb_in, sb_model_hidden_size, output_size, sequence_model)
        self._attach_holders()               # the submodules the forward calls are callable stages, like the reference's
        self.sequence_model = sequence_model

        self.subband_num = subband_num
        self.sb_num_neighbors = sb_num_neighbors
        self.fb_num_neighbors = fb_num_neighbors
        self.look_ahead = look_ahead
        self.norm_type = norm_type
        self.num_groups_in_drop_band = num_groups_in_drop_band
        self.output_size = output_size
        self.num_freqs = num_freqs
        self.kersize = list(kersize)
        self.fb_output_activate_function = fb_output_activate_function
        self.sb_output_activate_function = sb_output_activate_function
        self.sb_model_hidden_size = sb_model_hidden_size
        self._init_hip()
        if weight_init:
            self.apply(self.weight_init)          # fullsubnet_plus.py:119-120

    # ------------------------------------------------------------------ handle / weights
    def _config(self):
        cfg = self._common_config()
        cfg.tcn_hidden = 512
        cfg.num_tcn_blocks = len(_TCN_DILATIONS)
        for i, k in enumerate(self.kersize):
            cfg.kersize[i] = int(k)
        cfg.attention = _lib.ATTENTION[self.channel_attention_model]
        cfg.subband_num = self.subband_num
        return cfg

    # ------------------------------------------------------------------ forward
    def forward(self, noisy_mag, noisy_real, noisy_imag, batch_offset=0, global_batch=None, lengths=None):
        """
        Shapes:
            noisy_mag / noisy_real / noisy_imag: [B, 1, F, T] fp32 CUDA tensors (any strides)
            return: [B, 2, F, T]   (B == 1 or batch_mode == "full")
                    [B, 2, F//2, T] with the reference's drop_band row order (B > 1, batch_mode == "parity")
        batch_offset / global_batch: only for sharded batches (fullsubnet_plus_amd.dist).
        lengths: None, or frames per utterance (a Python sequence or a CPU integer tensor, 1 <= lengths[b] <= T) for a batch of
            clips of different lengths (batch_mode "full" only): row b is then, at frames [0, lengths[b]), the forward of
            x[b:b+1, ..., :lengths[b]] alone, and exactly 0 at frames [lengths[b], T).  Input frames past lengths[b] are never read.
        """
        return self._checked(lambda: self._forward_impl([noisy_mag, noisy_real, noisy_imag], batch_offset, global_batch, lengths=lengths))

    def _not_streamable(self, opener):
        from .stream import PLUS_REASON
        raise NotImplementedError(f"{self.__class__.__name__}.{opener}: {PLUS_REASON}")

    def open_stream(self, slots, max_chunk=16, device="cuda", live=False):
        """FullSubNet+ is not streamable (see fullsubnet_plus_amd.stream): always raises NotImplementedError with the reason."""
        self._not_streamable("open_stream")

    def open_wave_stream(self, slots, max_samples=4096, device="cuda", live=False, sample_rate=None):
        """FullSubNet+ is not streamable (see fullsubnet_plus_amd.stream): always raises NotImplementedError with the reason."""
        self._not_streamable("open_wave_stream")

    def open_spec_stream(self, slots, max_chunk=16, device="cuda", live=False):
        """FullSubNet+ is not streamable (see fullsubnet_plus_amd.stream): always raises NotImplementedError with the reason."""
        self._not_streamable("open_spec_stream")


class _FullBandLSTMParams(_StageHolder):
    """Parameter holder named like SequenceModel(sequence_model="LSTM") of the original FullSubNet's full-band model
    (fullsubnet/model/fullsubnet.py:39-47; sequence_model.py:31-38,78-79)."""

    def __init__(self, num_freqs, hidden, kind="LSTM"):
        super().__init__()
        rnn = nn.LSTM if kind == "LSTM" else nn.GRU
        self.sequence_model = rnn(num_freqs, hidden, num_layers=2, batch_first=True)
        self.fc_output_layer = nn.Linear(hidden, num_freqs)


class FullSubNet(_HipModel):
    """the original FullSubNet ``Model`` (speech_enhance/fullsubnet/model/fullsubnet.py:12-118, the
    commented alternative of config/inference.toml:11,28) on the same HIP kernels: constructor kwargs
    fullsubnet.py:13-26, ``forward(noisy_mag) -> [B, 2, F, T]`` fullsubnet.py:68-118, strict state_dict."""

    def __init__(self,
                 num_freqs,
                 look_ahead,
                 sequence_model,
                 fb_num_neighbors,
                 sb_num_neighbors,
                 fb_output_activate_function,
                 sb_output_activate_function,
                 fb_model_hidden_size,
                 sb_model_hidden_size,
                 norm_type="offline_laplace_norm",
                 num_groups_in_drop_band=2,
                 weight_init=True,
                 ):
        super().__init__()
        assert sequence_model in ("GRU", "LSTM"), f"{self.__class__.__name__} only support GRU and LSTM."
        _check_norm_and_activations(norm_type, fb_output_activate_function, sb_output_activate_function)
        self.fb_model = _FullBandLSTMParams(num_freqs, fb_model_hidden_size, sequence_model)
        self.sb_model = _SubBandParams((sb_num_neighbors * 2 + 1) + (fb_num_neighbors * 2 + 1), sb_model_hidden_size, 2,
                                       sequence_model)
        self._attach_holders()
        self.sequence_model = sequence_model

        self.sb_num_neighbors = sb_num_neighbors
        self.fb_num_neighbors = fb_num_neighbors
        self.look_ahead = look_ahead
        self.norm_type = norm_type
        self.num_groups_in_drop_band = num_groups_in_drop_band
        self.num_freqs = num_freqs
        self.output_size = 2
        self.fb_output_activate_function = fb_output_activate_function
        self.sb_output_activate_function = sb_output_activate_function
        self.fb_model_hidden_size = fb_model_hidden_size
        self.sb_model_hidden_size = sb_model_hidden_size
        self._init_hip()
        if weight_init:
            self.apply(self.weight_init)          # fullsubnet.py:65-66

    def _config(self):
        cfg = self._common_config()
        cfg.model = _lib.MODEL_FULLSUBNET
        cfg.tcn_hidden = self.fb_model_hidden_size       # fb_model_hidden_size (fsnp.h: FSNP_MODEL_FULLSUBNET)
        cfg.num_tcn_blocks = 0
        for i in range(3):
            cfg.kersize[i] = 1
        cfg.attention = 0
        return cfg

    def forward(self, noisy_mag, batch_offset=0, global_batch=None, lengths=None):
        """noisy_mag [B, 1, F, T] fp32 CUDA tensor (any strides) -> cIRM [B, 2, F, T] (see FullSubNet_Plus.forward
        for batch_mode, the sharding arguments and lengths)."""
        return self._checked(lambda: self._forward_impl([noisy_mag], batch_offset, global_batch, lengths=lengths))

    def open_stream(self, slots, max_chunk=16, device="cuda", live=False):
        """-> fullsubnet_plus_amd.stream.Stream: `slots` independent live streams that are fed a few frames per push and carry the
        recurrent state and the cumulative norms' sums between pushes (include/fsnp_stream.h).  A clip pushed in any chunking, followed
        by tail(), gives forward()'s mask of that clip delayed by look_ahead columns.  Needs a cumulative norm and LSTM cells
        (NotImplementedError with the reason otherwise, before any GPU is touched).

        live=True opens a LIVE session (include/fsnp_stream_live.h): the mode for a few calls fed one hop at a time.  Its pushes run the
        two recurrent models as one short launch per layer and step, cut by columns over the whole chip, where a default session keeps
        one launch each resident over the chunk (one 32-row tile per CU, one workgroup for the full-band model of one slot).  Same
        interface and state records (state() of one mode loads into the other); max_chunk <= 16.  Measured on one MI355X
        (profiles/stream_throughput.md, ms per push at n = 1, default -> live): 1 slot 0.47 -> 0.14, 8 slots 0.48 -> 0.26, 32 slots
        0.72 -> 0.57, 64 slots 0.97 -> 1.03: open a live session up to 32 slots, a default one from 64 slots on or for longer chunks."""
        from .stream import Stream, refusal
        why = refusal(self)
        if why is not None:
            raise NotImplementedError(f"{self.__class__.__name__}.open_stream: {why}")
        return Stream(self, slots, max_chunk, _resolve_device(device), live=live)

    def open_wave_stream(self, slots, max_samples=4096, device="cuda", live=False, sample_rate=None):
        """-> fullsubnet_plus_amd.stream.WaveStream: `slots` independent live audio streams, blocks of up to max_samples samples in, as
        many enhanced samples out at the fixed delay n_fft + look_ahead * hop_length (include/fsnp_wave_stream.h; (2 + look_ahead) * hop
        in the default geometry).  The session runs at the model's hop_length of this moment and keeps it.  All push outputs of a clip
        followed by finish(), without the first `delay` samples, are enhance_wave() of that clip alone.  The refusals of open_stream
        apply (NotImplementedError with the reason, before any GPU is touched).  live=True: the model inside runs as a live session
        (see open_stream); max_samples / hop + 1 frames per push must then be <= 16, e.g. max_samples = hop for one hop per push, and so
        must the ceil(n_fft / (2 hop)) + look_ahead frames of a finish.

        sample_rate (include/fsnp_wave_rate_stream.h): None or self.sample_rate is the session as it has always been.  Any other rate
        in Hz -> fullsubnet_plus_amd.stream.WaveRateStream: blocks at that rate in, as many samples at that rate out, converted to and
        from self.sample_rate on the device inside every push by the filter of enhance_wave(..., sample_rate=); max_samples then counts
        at that rate, and so does the session's `delay` (68 ms at 48 kHz where the model's own is 64 ms).  A live session's 16 frames
        per call apply to the model-rate samples a push turns into (`model_max_samples`): at 48 kHz, hop 256 and one 10 ms block per
        push, max_samples = 480.  ValueError, before any GPU is touched, for a rate that is no positive integer or a ratio with
        max(up, down) > 640."""
        from .stream import WaveRateStream, WaveStream, wave_refusal
        what = f"{self.__class__.__name__}.open_wave_stream"
        why = wave_refusal(self)
        if why is not None:
            raise NotImplementedError(f"{what}: {why}")
        rate = other_rate(sample_rate, self.sample_rate, what)
        if rate is not None:
            return WaveRateStream(self, slots, max_samples, _resolve_device(device), live=live, sample_rate=rate)
        return WaveStream(self, slots, max_samples, _resolve_device(device), live=live)

    def open_spec_stream(self, slots, max_chunk=16, device="cuda", live=False):
        """-> fullsubnet_plus_amd.stream.SpecStream: `slots` independent live streams for a caller who owns the STFT (any window, any
        overlap): up to max_chunk noisy complex64 frames in, as many enhanced frames out, look_ahead frames late
        (include/fsnp_spec_stream.h).  The noisy frames wait for their masks inside the slot's state, which state() / load_state carry
        whole.  A clip pushed in any chunking, followed by tail(), gives [look_ahead zero columns | enhance() of that clip alone].  The
        refusals of open_stream apply (NotImplementedError with the reason, before any GPU is touched).  live=True: the model inside
        runs as a live session (see open_stream); max_chunk <= 16."""
        from .stream import SpecStream, spec_refusal
        why = spec_refusal(self)
        if why is not None:
            raise NotImplementedError(f"{self.__class__.__name__}.open_spec_stream: {why}")
        return SpecStream(self, slots, max_chunk, _resolve_device(device), live=live)


Model = FullSubNet_Plus  # the name BASELINE.json's north_star uses
