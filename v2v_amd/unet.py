"""The recurrent UNet that consumes the voxel grids (BASELINE config 5), assembled from the device kernels of
v2v_amd/convlstm.py under the REFERENCE'S OWN module tree, so that a reference checkpoint loads unchanged:

    E2VIDRecurrent(unet_kwargs)            model/model.py:194-223          keys  unetrecurrent.*
    UNetRecurrent(unet_kwargs)             model/unet.py:252-310           keys  head.conv2d.*, encoders.N.conv.conv2d.*,
                                                                                 encoders.N.recurrent_block.Gates.*,
                                                                                 resblocks.N.conv1.* / conv2.*,
                                                                                 decoders.N.conv2d.*, pred.conv2d.*
    RecurrentConvLayer / UpsampleConvLayer model/submodules.py:99-119 / :68-96

    FlowNet(unet_kwargs)                   model/model.py:111-139          keys  unetflow.*   (E2VID+: {'image', 'flow'})
    FireNet(num_bins, base_num_channels, kernel_size, unet_kwargs)   model/model.py:264-311   keys  head / G1 / R1 / G2 / R2 / pred
    UNetFlow(unet_kwargs)                  model/unet.py:133-194           UNetRecurrent's body at prediction width 3

Configuration covered = what config/train_v2v_e2vid_10k.yaml:21-30 / config/test_e2vid++_original.yaml instantiate: skip_type 'sum',
recurrent_block_type 'convlstm' or (E2VIDRecurrent / FlowNet, inference only) 'convgru', use_upsample_conv true, norm none, kernel_size 5, base_num_channels 32, channel_multiplier 2 (anything else raises:
there is no stock-layer fallback inside this module).  Inference by default; trainable=True adds the backward kernels of
v2v_amd/train.py (back-propagation through time through the ConvLSTM states when grad is enabled).

    EVFlowNet(unet_kwargs)                 model/model.py:226-261          keys  unet.*
    UNet(unet_kwargs)                      model/unet.py:313-352           keys  encoders.N.conv2d.*, resblocks.N.conv1.* / conv2.*,
                                                                                 decoders.N.conv2d.*, pred.conv2d.*
(the stateless flow network of config/train_v2v_evflow_10k.yaml / config/test_evflow_original.yaml: skip_type 'concat', kernel_size 3,
norm none, use_upsample_conv true, base 32, 4 encoders, multiplier 2; anything else raises).

Inside forward() everything runs in bfloat16 NHWC (torch.channels_last views of the kernels' own buffers): the head takes
the float voxel grid in any layout, every later layer consumes and produces NHWC in place, the cell states stay float32, and
the prediction comes back in the input's dtype.  Parity: golden G18 = the reference's modules run in float32 on seeded
weights (tests/test_unet_golden.py; tolerance stated there).

Shared by the sequence calls: _sequence_shape (the [N,T,bins,H,W] check), _t_major (one launch of a state-free layer for all T steps),
_Stateful (states / reset_states / the hipGraph capture of a sequence: E2VIDRecurrent, FlowNet and FireNet) and _graphed_sequence behind it.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .convlstm import ConvGRU, ConvLayer, ConvLSTM, ResidualBlock, _out_dtype, clone_state
from .nhwc_ops import tile_like_batch


def _sequence_shape(events):
    """(N, T) of an [N, T, num_bins, H, W] sequence; anything else raises."""
    if events.dim() != 5:
        raise ValueError("events must be [N, T, num_bins, H, W]")
    return events.shape[0], events.shape[1]


def _t_major(events, event_scales):
    """What a layer that does not touch the states needs to run for all T steps in ONE launch: (events as [T*N, num_bins, H, W], the scales
    repeated to match | None, step) with step(batched, t) = the rows of time step t (t*N .. (t+1)*N) of anything computed from them."""
    n, t_steps = events.shape[:2]
    ev_t = events.transpose(0, 1).reshape((t_steps * n,) + tuple(events.shape[2:]))
    sc_t = event_scales.repeat(t_steps, 1) if event_scales is not None else None
    return ev_t, sc_t, lambda batched, t: batched[t * n:(t + 1) * n]


class UpsampleConvLayer(ConvLayer):
    """model/submodules.py:68-96: bilinear x2 upsampling + convolution + ReLU; forward(x, skip) == forward(skip_sum(x, skip))."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation="relu", norm=None, trainable: bool = False):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, activation=activation, norm=norm,
                         upsample=True, trainable=trainable)


class RecurrentConvLayer(nn.Module):
    """model/submodules.py:99-119: ConvLayer followed by the ConvLSTM or the ConvGRU; same attribute names (`conv`, `recurrent_block`).
    forward returns (x, state): state = (hidden, cell) and x = hidden for 'convlstm', state = x = the new hidden state for 'convgru' (:117)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, recurrent_block_type="convlstm",
                 activation="relu", norm=None, BN_momentum=0.1, trainable: bool = False):
        super().__init__()
        if recurrent_block_type not in ("convlstm", "convgru"):
            raise ValueError("recurrent_block_type is 'convlstm' or 'convgru' (model/submodules.py:104)")
        if recurrent_block_type == "convgru" and trainable:
            raise ValueError("trainable=True with recurrent_block_type 'convgru': the ConvGRU step has no backward kernel yet "
                             "(train with 'convlstm', or build the network with trainable=False)")
        self.recurrent_block_type = recurrent_block_type
        self.conv = ConvLayer(in_channels, out_channels, kernel_size, stride, padding, activation, norm, trainable=trainable)
        block = ConvLSTM if recurrent_block_type == "convlstm" else ConvGRU
        self.recurrent_block = block(input_size=out_channels, hidden_size=out_channels, kernel_size=3, trainable=trainable)

    def forward(self, x, prev_state, conv_out=None):
        """conv_out (this implementation only): self.conv(x) when the caller has it already -- the convolution does not touch the state,
        so UNetRecurrent.forward_sequence runs the first encoder's for all time steps in one launch."""
        x = self.conv(x) if conv_out is None else conv_out  # ReLU in the convolution's epilogue
        state = self.recurrent_block(x, prev_state)
        return (state[0] if self.recurrent_block_type == "convlstm" else state), state


class UNetRecurrent(nn.Module):
    """model/unet.py:252-310 (+ BaseUNet :13-64).  `unet_kwargs` as the reference's YAML gives them.  trainable=True: every layer records
    its backward (v2v_amd/train.py) when grad is enabled; with grad disabled, or trainable=False, the network is the inference one."""

    NUM_OUTPUT_CHANNELS = 1                                # :263 -- the prediction width (UNetFlow: 3)

    def __init__(self, unet_kwargs, trainable: bool = False, convgru: bool = False):
        """convgru: recurrent_block_type 'convgru' is an opt-in of the caller.  This class on its own keeps refusing it, as it always has
        (a ConvGRU state is one tensor carrying a float32 master, not the (hidden, cell) pair code written against this class expects);
        the model classes E2VIDRecurrent and FlowNet, which own the states and copy them with their masters, opt in."""
        super().__init__()
        self.trainable = bool(trainable)
        kw = dict(unet_kwargs)
        final_activation = kw.pop("final_activation", "none")
        self.final_activation = getattr(torch, final_activation, None) if final_activation else None
        kw["num_output_channels"] = self.NUM_OUTPUT_CHANNELS
        self.base_num_channels = kw["base_num_channels"]
        self.num_encoders = kw["num_encoders"]
        self.num_residual_blocks = kw["num_residual_blocks"]
        self.num_output_channels = kw["num_output_channels"]
        self.kernel_size = kw.get("kernel_size", 5)
        self.skip_type = kw["skip_type"]
        self.norm = kw.get("norm", None)
        self.num_bins = kw["num_bins"]
        self.recurrent_block_type = kw.get("recurrent_block_type", None)
        if self.recurrent_block_type == "convgru" and not convgru:
            raise ValueError("recurrent_block_type 'convgru' runs through the model classes (E2VIDRecurrent, FlowNet), or with convgru=True: "
                             "its state is one tensor with a float32 master (v2v_amd.unet.copy_states keeps it)")
        mult = kw.get("channel_multiplier", 2)
        if self.norm in ("none", "None", ""):
            self.norm = None
        if self.skip_type != "sum" or not kw.get("use_upsample_conv", True) or self.norm is not None:
            raise ValueError("the device kernels cover skip_type 'sum', use_upsample_conv true, norm none "
                             "(config/train_v2v_e2vid_10k.yaml:21-30)")
        self.encoder_input_sizes = [int(self.base_num_channels * pow(mult, i)) for i in range(self.num_encoders)]
        self.encoder_output_sizes = [int(self.base_num_channels * pow(mult, i + 1)) for i in range(self.num_encoders)]
        self.max_num_channels = self.encoder_output_sizes[-1]
        k = self.kernel_size
        self.head = ConvLayer(self.num_bins, self.base_num_channels, kernel_size=k, stride=1, padding=k // 2, trainable=trainable)
        self.head.force_channels_last = True               # NHWC from the first layer on, whatever layout the voxel grid arrives in
        self.encoders = nn.ModuleList(
            RecurrentConvLayer(i, o, kernel_size=k, stride=2, padding=k // 2, recurrent_block_type=self.recurrent_block_type, norm=self.norm,
                               trainable=trainable)
            for i, o in zip(self.encoder_input_sizes, self.encoder_output_sizes))
        for enc in self.encoders:
            enc.recurrent_block.wants_skip_twin = True         # training: the decoder's skip reads its own output of the step (fp32 dh sum)
        self.resblocks = nn.ModuleList(ResidualBlock(self.max_num_channels, self.max_num_channels, norm=self.norm, trainable=trainable)
                                       for _ in range(self.num_residual_blocks))
        self.decoders = nn.ModuleList(UpsampleConvLayer(i, o, kernel_size=k, padding=k // 2, norm=self.norm, trainable=trainable)
                                      for i, o in zip(reversed(self.encoder_output_sizes), reversed(self.encoder_input_sizes)))
        self.pred = ConvLayer(self.base_num_channels, self.num_output_channels, 1, activation=None, norm=self.norm, trainable=trainable)
        self.states = [None] * self.num_encoders

    def _encode(self, x, event_scales, head=None, conv0=None):
        """head + the recurrent encoders of one time step (model/unet.py:287-296) -> (head, blocks): everything that touches the states.
        `head` / `conv0`: the head layer's and the first encoder convolution's outputs for this step when the caller computed them
        already (forward_sequence does, for all steps at once: neither depends on the states)."""
        if head is None:
            with torch.autocast("cuda", dtype=torch.bfloat16):  # the head hands out bfloat16; every later layer keeps it
                head = self.head(x, scales=event_scales)        # reads any strides (its own layout kernel), bfloat16 NHWC out
        x = head
        blocks = []
        for i, encoder in enumerate(self.encoders):
            x, state = encoder(x, self.states[i], conv_out=conv0 if i == 0 else None)
            blocks.append(encoder.recurrent_block.skip_twin(x))
            self.states[i] = state
        if blocks[-1] is not x:                                 # training: the skips are the steps' twin outputs; the residual blocks
            blocks.append(x)                                    # read blocks[-1] = the last hidden state itself (_decode)
        return head, blocks

    def _decode(self, head, blocks):
        """residual blocks + decoders + prediction of one time step (model/unet.py:298-309): stateless."""
        x = blocks[-1]
        for resblock in self.resblocks:
            x = resblock(x)
        for i, decoder in enumerate(self.decoders):
            x = decoder(x, blocks[self.num_encoders - i - 1])   # skip_sum folded into the upsampling kernel (:304)
        img = self.pred(x, head)                                 # pred(skip_sum(x, head)) in one pass (:307)
        if self.final_activation is not None:
            img = self.final_activation(img)
        return img

    def _pack_weights(self):
        """Every layer's packed weight copy made (or found current) on the CALLER's stream.  The layers pack lazily inside forward(); a first
        call, or one after load_state_dict / a weight update, would otherwise pack the decoder halves' weights on the side stream of step
        0 -- and step 1's decoder half, on ANOTHER side stream ordered only after the caller's `ready` event, could read them before the
        pack kernels have written them (and the packed tensors would live in one side stream's allocator pool while every stream reads
        them).  Packed here, they are ordered before every side stream by the wait_stream() that follows."""
        for m in self.modules():
            if hasattr(type(m), "_weights"):                    # the layers' protocol: everything forward needs packed, now
                m._weights()

    def forward_sequence(self, events, event_scales=None, out=None, overlap=True):
        """The time loop of model/train_utils.py:339-345 (`for t in range(T): pred = model(events[:, t]); pred_imgs[:, t] = pred['image']`)
        as ONE call: events [N,T,num_bins,H,W] -> predictions [N,T,num_output_channels,H,W] (events' dtype, or `out`), the states advanced by T steps.

        The recurrence only runs through the encoders' ConvLSTM states; residual blocks, decoders and prediction of step t are stateless.
        With overlap they are issued on side HIP streams (overlap=True: three, taken in turn by consecutive steps; an int: that many),
        so step t's decoder half runs UNDER step t+1's encoder half and beside its neighbours' decoder halves: at the training shape
        (12 x 128 x 128) no single layer fills 256 CUs (48-384 workgroups), and half-filling kernels side by side use what one leaves
        idle (ms per time step, hipGraph replay, tools/e2vid_pipeline_probe.py: loop 0.50, one side stream 0.37, two 0.355, three 0.34;
        0.316 with the state-free layers batched over time, below).  Same kernels on the same operands in the same per-tensor order:
        results are bit-identical to the step-by-step loop (tests/test_unet_golden.py).
        Stream-ordering contract with torch's caching allocator: tensors made on the caller's stream and read on the side stream
        (head, skip blocks) are kept alive until the caller's stream has waited for the side stream's event of that step, so a freed
        block can never be handed out again while the side stream still reads it.  Captures into a hipGraph (fork / join through
        events) like the single-stream loop.  (A three-STAGE form -- the decoder half itself split over two chained side streams -- ran
        eagerly but crashed hipGraph's capture_end on ROCm 7.2; whole decoder halves on alternating streams capture fine.)"""
        n, t_steps = _sequence_shape(events)
        if out is None:
            out = torch.empty((n, t_steps, self.num_output_channels) + tuple(events.shape[-2:]), dtype=_out_dtype(events), device=events.device)
        if self.trainable and torch.is_grad_enabled():
            overlap = False                                     # training: the plain step loop (autograd records every step on this stream)
        if not overlap:
            for t in range(t_steps):
                head, blocks = self._encode(events[:, t], event_scales)
                out[:, t] = self._decode(head, blocks)
            return out
        # The head layer and the first encoder's convolution do not touch the states: all T steps' in ONE well-filled launch each (T*N
        # images) instead of T small ones on the critical path of the recurrence (0.339 -> 0.322 -> 0.30 ms per step at the training
        # shape).  Per image the kernels do the same work whatever the batch is, so the values are those of the per-step calls bit for
        # bit.  Capped at 2 GiB of bf16 activations (heads: 32 channels at full resolution; conv0: 64 at half).
        heads = conv0s = None
        c_head = self.base_num_channels
        if t_steps > 1 and n * t_steps * events.shape[-2] * events.shape[-1] * c_head * 3 <= (2 << 30):
            ev_t, sc_t, step = _t_major(events, event_scales)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                heads = self.head(ev_t, scales=sc_t)
                if n * events.shape[-2] * events.shape[-1] <= 16 * 128 * 128:   # larger steps fill the chip themselves (8 x 256^2: batching the
                    conv0s = self.encoders[0].conv(heads)                      # convolution measured 0.690 -> 0.70 ms per step, it stays per step)
            del ev_t, sc_t
        cur = torch.cuda.current_stream(events.device)
        n_side = 3 if overlap is True else max(1, int(overlap))  # decoder halves of consecutive steps alternate between the side streams
        pool = self.__dict__.setdefault("_side_streams", {})
        key = (events.device, n_side)
        if key not in pool:
            pool[key] = [torch.cuda.Stream(device=events.device) for _ in range(n_side)]
        sides = pool[key]
        self._pack_weights()                                    # on `cur`, BEFORE the fork: see _pack_weights
        for side in sides:
            side.wait_stream(cur)                               # `out`, the weights' packed copies, whatever the caller queued before
        held = []                                               # (tensors of a step a side stream reads, its completion event)
        for t in range(t_steps):
            if len(held) == n_side + 1:                         # the oldest step's operands may go once cur is ordered after their last reader
                cur.wait_event(held[0][1])
                held.pop(0)
            head, blocks = self._encode(events[:, t], event_scales, head=None if heads is None else step(heads, t),
                                        conv0=None if conv0s is None else step(conv0s, t))
            ready = torch.cuda.Event()
            ready.record(cur)
            side = sides[t % n_side]
            with torch.cuda.stream(side):
                side.wait_event(ready)
                out[:, t] = self._decode(head, blocks)
                done = torch.cuda.Event()
                done.record(side)
            held.append(((head, blocks), done))
        for side in sides:
            cur.wait_stream(side)
        return out

    def forward(self, x, event_scales=None):
        """x: [N, num_bins, H, W] float voxel grid (any layout), H and W multiples of 16 (what forward_sequence pads to, model/train_utils.py:322-326; anything else raises) -> {'image': [N,1,H,W]}.
        event_scales (this implementation only): float32 [N,2] = (neg_max, pos_max) per sample, e.g. RingLoader(normalize='scales')'s
        batch['event_scales'] -- normalize_batch_voxel (model/train_utils.py:147-166) is then applied by the head while it reads the
        RAW voxel grid; None = x is used as it is."""
        out_dtype = _out_dtype(x)
        head, blocks = self._encode(x, event_scales)
        return {"image": self._decode(head, blocks).to(out_dtype)}


def copy_states(states):
    """model/model.py:17-24 copy_states: clone every state tensor (a list of None stays a list of None)
    (a ConvGRU state -- a single tensor -- keeps its float32 master: convlstm.clone_state)."""
    if states[0] is None:
        return list(states)
    return [tuple(s.detach().clone() for s in st) if isinstance(st, tuple) else clone_state(st) for st in states]


class UNetFlow(UNetRecurrent):
    """model/unet.py:133-194: the recurrent UNet with a 3-channel prediction -- UNetRecurrent's body at prediction width 3 (same module tree,
    same keys) -- returning {'image': [:, 0:1], 'flow': [:, 1:3]}.  (img_3c and final_activation are not part of it: :140-159.)"""

    NUM_OUTPUT_CHANNELS = 3                                # :141

    def __init__(self, unet_kwargs, trainable: bool = False, convgru: bool = True):
        if "final_activation" in unet_kwargs:
            raise ValueError("UNetFlow takes no final_activation (model/unet.py:140-142 passes its kwargs to BaseUNet, which has none)")
        super().__init__(unet_kwargs, trainable=trainable, convgru=convgru)

    @staticmethod
    def split(img_flow):
        """[..., 3, H, W] -> {'image': [..., 0:1, H, W], 'flow': [..., 1:3, H, W]} (:192), views of the prediction."""
        return {"image": img_flow[..., 0:1, :, :], "flow": img_flow[..., 1:3, :, :]}

    def forward(self, x, event_scales=None):
        return self.split(super().forward(x, event_scales)["image"])


def _graphed_sequence(owner, events, event_scales, extra_key, run, get_states, set_states):
    """The hipGraph capture / replay behind forward_sequence(graph=True) of the recurrent model classes: run(ev, sc) -- reset the states, then
    the whole sequence on the graph's static input buffers -- is captured ONCE per (shape, dtype, device, extra_key, weights) and replayed
    from then on; get_states() / set_states(list) read and assign the owner's live state list (the graph's own state tensors are what the
    last captured step wrote).  One live graph per owner: a new shape or new weights retire the old one and its buffers."""
    params = list(owner.parameters())
    key = (tuple(events.shape), events.dtype, events.device, event_scales is not None, extra_key,
           tuple(p.data_ptr() for p in params), sum(p._version for p in params))
    cache = owner.__dict__.setdefault("_sequence_graphs", {})
    entry = cache.get(key)
    if entry is None:
        cache.clear()
        ev = torch.empty_like(events, memory_format=torch.contiguous_format)
        sc = torch.empty_like(event_scales, memory_format=torch.contiguous_format) if event_scales is not None else None
        ev.copy_(events)
        if sc is not None:
            sc.copy_(event_scales)
        with torch.no_grad():
            run(ev, sc)                                         # eager once: weight packing, LDS-size attributes, allocator warm-up
            torch.cuda.synchronize(events.device)
            warm = torch.cuda.Stream(device=events.device)
            warm.wait_stream(torch.cuda.current_stream(events.device))
            with torch.cuda.stream(warm):
                run(ev, sc)
            torch.cuda.current_stream(events.device).wait_stream(warm)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                res = run(ev, sc)
        entry = cache[key] = (g, ev, sc, res, tuple(get_states()))   # an immutable copy: eager calls between two replays assign into the live list
    g, ev, sc, res, states = entry
    ev.copy_(events)
    if sc is not None:
        sc.copy_(event_scales)
    g.replay()
    set_states(list(states))                                    # the graph's own state tensors: what the last captured step wrote
    return res


class _Stateful(nn.Module):
    """What every model class with recurrent states shares: the `states` property (copies out, assigns in) / reset_states the reference's
    training loop uses, and the hipGraph capture of a whole sequence.  `_states` is the live list of `num_recurrent_units` states: an
    attribute of the model itself (FireNet) or a property forwarding to its network's (_RecurrentModel)."""

    @property
    def states(self):
        return copy_states(self._states)

    @states.setter
    def states(self, states):
        self._states = states

    def reset_states(self):
        self._states = [None] * self.num_recurrent_units

    def _graphed(self, events, event_scales, extra_key, sequence):
        """forward_sequence(graph=True): reset_states(), then sequence(ev, sc), captured once and replayed (_graphed_sequence)."""
        def run(ev, sc):
            self.reset_states()
            return sequence(ev, sc)
        return _graphed_sequence(self, events, event_scales, extra_key, run, lambda: self._states, lambda st: setattr(self, "_states", st))


class _RecurrentModel(_Stateful):
    """What the reference's recurrent model classes share (model/model.py:194-223, :111-139): the network under its own attribute name
    (`NET`), which owns the states, the sequence call and its hipGraph capture."""

    NET = None                                             # attribute (and state_dict prefix) of the network
    NET_CLASS = None

    def __init__(self, unet_kwargs, trainable: bool = False):
        super().__init__()
        self.num_bins = unet_kwargs["num_bins"]
        self.num_encoders = self.num_recurrent_units = unet_kwargs["num_encoders"]
        self.trainable = bool(trainable)           # the YAML switch: model: {target: .., params: {unet_kwargs: .., trainable: true}}
        setattr(self, self.NET, self.NET_CLASS(unet_kwargs, trainable=trainable, convgru=True))

    @property
    def net(self):
        return getattr(self, self.NET)

    @property
    def _states(self):
        return self.net.states

    @_states.setter
    def _states(self, states):
        self.net.states = states

    def forward(self, event_tensor, event_scales=None):
        return self.net.forward(event_tensor, event_scales)

    def forward_sequence(self, events, event_scales=None, out=None, overlap=True, graph=False):
        """[N,T,num_bins,H,W] -> [N,T,num_output_channels,H,W]: the reference's time loop (model/train_utils.py:339-345) in one call, decoder half of step t
        under the encoder half of step t+1 (UNetRecurrent.forward_sequence).

        graph=True: the whole sequence -- reset_states() first, as forward_sequence(reset_states=True) does (model/train_utils.py:309-313),
        then T steps on the overlapped streams -- is captured ONCE per (shape, dtype, device, weights) into a hipGraph and replayed from
        then on: ~20 launches per time step cost the host ~12 ms per 40-step sequence when issued one by one, about what the GPU needs to
        run them.  Inputs are copied into the graph's static buffers; the returned tensor is the graph's static output (overwritten by
        the next call with the same shapes -- clone it to keep it); the states after the call are those of the sequence's last step.
        Inference only (with trainable=True and grad enabled: ValueError)."""
        if not graph:
            return self.net.forward_sequence(events, event_scales, out=out, overlap=overlap)
        if self.trainable and torch.is_grad_enabled():
            raise ValueError("graph=True captures inference only: run training steps with graph=False (or under torch.no_grad())")
        if out is not None:
            raise ValueError("graph=True returns the captured graph's own output buffer; `out` is not supported")
        return self._graphed(events, event_scales, overlap, lambda ev, sc: self.net.forward_sequence(ev, sc, overlap=overlap))


class E2VIDRecurrent(_RecurrentModel):
    """model/model.py:194-223: `unetrecurrent` + the states property / reset_states the training loop uses.  Both recurrent block types;
    'convgru' is inference-only."""

    NET, NET_CLASS = "unetrecurrent", UNetRecurrent


class FlowNet(_RecurrentModel):
    """model/model.py:111-139: `unetflow` = UNetFlow, the E2VID+ network of config/test_e2vid++_original.yaml; keys unetflow.*.
    forward -> {'image': [N,1,H,W], 'flow': [N,2,H,W]}; forward_sequence -> {'image': [N,T,1,H,W], 'flow': [N,T,2,H,W]} (views of one
    [N,T,3,H,W] tensor; graph=True: of the captured graph's static output).  Both recurrent block types; trainable=True with 'convlstm'."""

    NET, NET_CLASS = "unetflow", UNetFlow

    def forward_sequence(self, events, event_scales=None, out=None, overlap=True, graph=False):
        return UNetFlow.split(super().forward_sequence(events, event_scales, out=out, overlap=overlap, graph=graph))


class FireNet(_Stateful):
    """model/model.py:264-311: the reference's light reconstruction network, head ConvLayer(num_bins -> 16, 3x3, relu), G1 = ConvGRU(16, 16, 3),
    R1 = ResidualBlock(16, 16), G2, R2, pred = ConvLayer(16 -> 1, 1x1), every layer at full resolution -- on the 16-channel kernels of
    v2v_amd/csrc/v2v_narrow.hpp (each ConvGRU step and each residual block is ONE launch).  Same constructor (the legacy `unet_kwargs`
    override included), same module tree: the 24 keys of a reference checkpoint load with strict=True.  Nothing leaves NHWC bfloat16 between
    head and prediction; the two hidden states are carried in float32 beside their bfloat16 copies (ConvGRU).  Any H and W: there is no
    stride, so frames run unpadded.  Inference only: base_num_channels != 16, kernel_size != 3 and trainable=True raise."""

    def __init__(self, num_bins=5, base_num_channels=16, kernel_size=3, unet_kwargs={}, trainable: bool = False):
        super().__init__()
        if unet_kwargs:                                        # legacy compatibility (model/model.py:272-275)
            num_bins = unet_kwargs.get("num_bins", num_bins)
            base_num_channels = unet_kwargs.get("base_num_channels", base_num_channels)
            kernel_size = unet_kwargs.get("kernel_size", kernel_size)
        if trainable:
            raise ValueError("FireNet is inference-only: the ConvGRU step has no backward kernel (trainable=True is not available)")
        if base_num_channels != 16 or kernel_size != 3 or not 1 <= num_bins <= 8:
            raise ValueError("the device kernels cover FireNet as the reference builds it: base_num_channels 16, kernel_size 3, num_bins <= 8 "
                             f"(got {base_num_channels}, {kernel_size}, {num_bins}); there is no stock-layer fallback")
        self.num_bins = num_bins
        self.trainable = False
        c = base_num_channels
        self.head = ConvLayer(num_bins, c, kernel_size, padding=kernel_size // 2)
        self.head.force_channels_last = True                   # NHWC from the first layer on, whatever layout the voxel grid arrives in
        self.G1 = ConvGRU(c, c, kernel_size)
        self.R1 = ResidualBlock(c, c)
        self.G2 = ConvGRU(c, c, kernel_size)
        self.R2 = ResidualBlock(c, c)
        self.pred = ConvLayer(c, 1, 1, activation=None)
        self.num_encoders = 0                                  # needed by the reference's image_reconstructor.py
        self.num_recurrent_units = 2
        self.reset_states()

    def _head(self, x, event_scales):
        with torch.autocast("cuda", dtype=torch.bfloat16):      # the head hands out bfloat16 NHWC; every later layer keeps it
            return self.head(x, scales=event_scales)

    def _body(self, x):
        """Everything behind the head for one time step (:305-311), on the head's output."""
        x = self._states[0] = self.G1(x, self._states[0])
        x = self.R1(x)
        x = self._states[1] = self.G2(x, self._states[1])
        x = self.R2(x)
        return self.pred(x)

    def forward(self, x, event_scales=None):
        """x: [N, num_bins, H, W] float voxel grid (any layout, any H and W) -> {'image': [N,1,H,W]} in x's dtype (bfloat16 under autocast).
        event_scales as in UNetRecurrent.forward: normalize_batch_voxel applied by the input staging kernel on the RAW voxel grid."""
        return {"image": self._body(self._head(x, event_scales)).to(_out_dtype(x))}

    def forward_sequence(self, events, event_scales=None, graph=False):
        """The reference's time loop (`for t in range(T): pred = model(events[:, t])`) as one call: events [N,T,num_bins,H,W] -> images
        [N,T,1,H,W].  The head does not touch the states: it runs for all T steps in one launch (per image the kernel does the same work
        whatever the batch is), then the step loop; the result equals the per-step loop bit for bit.  One linear stream: every layer depends
        on the one before it through the recurrent states, so there is nothing to overlap.
        graph=True: reset_states(), then the T steps, captured once per (shape, dtype, device, weights) into a hipGraph and replayed from
        then on (as E2VIDRecurrent.forward_sequence): the returned tensor is the graph's static output (clone it to keep it)."""
        n, t_steps = _sequence_shape(events)
        if graph:
            return self._graphed(events, event_scales, None, self.forward_sequence)
        out = torch.empty((n, t_steps, 1) + tuple(events.shape[-2:]), dtype=_out_dtype(events), device=events.device)
        ev_t, sc_t, step = _t_major(events, event_scales)
        heads = self._head(ev_t, sc_t)
        for t in range(t_steps):
            out[:, t] = self._body(step(heads, t))
        return out


class UNet(nn.Module):
    """model/unet.py:313-352 (+ BaseUNet :13-64): the plain (stateless) UNet with concat skips, no head -- the first encoder reads the
    events.  Same attribute names (`encoders`, `resblocks`, `decoders`, `pred`), so a reference state_dict loads with strict=True.
    Covered: skip_type 'concat', kernel_size 3, norm none, use_upsample_conv true, base_num_channels 32, 4 encoders, channel_multiplier
    2, <= 8 bins, 1..3 outputs (what EVFlowNet hard-codes); anything else raises.  trainable=True records every layer's backward."""

    def __init__(self, unet_kwargs, trainable: bool = False):
        super().__init__()
        self.trainable = bool(trainable)
        kw = dict(unet_kwargs)
        self.base_num_channels = kw["base_num_channels"]
        self.num_encoders = kw["num_encoders"]
        self.num_residual_blocks = kw["num_residual_blocks"]
        self.num_output_channels = kw["num_output_channels"]
        self.kernel_size = kw.get("kernel_size", 5)
        self.skip_type = kw["skip_type"]
        self.norm = kw.get("norm", None)
        self.num_bins = kw["num_bins"]
        mult = kw.get("channel_multiplier", 2)
        if self.norm in ("none", "None", ""):
            self.norm = None
        if self.skip_type != "concat" or not kw.get("use_upsample_conv", True) or self.norm is not None or self.kernel_size != 3 \
                or self.base_num_channels != 32 or self.num_encoders != 4 or mult != 2 or not 1 <= self.num_bins <= 8 \
                or not 1 <= self.num_output_channels <= 3:
            raise ValueError("the device kernels cover the plain UNet as EVFlowNet builds it: skip_type 'concat', kernel_size 3, norm none, "
                             "use_upsample_conv true, base_num_channels 32, num_encoders 4, channel_multiplier 2, num_bins <= 8, <= 3 outputs "
                             "(model/model.py:234-245)")
        self.encoder_input_sizes = [int(self.base_num_channels * pow(mult, i)) for i in range(self.num_encoders)]
        self.encoder_output_sizes = [int(self.base_num_channels * pow(mult, i + 1)) for i in range(self.num_encoders)]
        self.max_num_channels = self.encoder_output_sizes[-1]
        k = self.kernel_size
        self.encoders = nn.ModuleList(
            ConvLayer(self.num_bins if n == 0 else i, o, kernel_size=k, stride=2, padding=k // 2, norm=self.norm, trainable=trainable)
            for n, (i, o) in enumerate(zip(self.encoder_input_sizes, self.encoder_output_sizes)))   # encoders[0] = the stem (:322)
        self.encoders[0].force_channels_last = True        # NHWC from the first layer on, whatever layout the voxel grid arrives in
        self.resblocks = nn.ModuleList(ResidualBlock(self.max_num_channels, self.max_num_channels, norm=self.norm, trainable=trainable)
                                       for _ in range(self.num_residual_blocks))
        self.decoders = nn.ModuleList(UpsampleConvLayer(2 * i, o, kernel_size=k, padding=k // 2, norm=self.norm, trainable=trainable)
                                      for i, o in zip(reversed(self.encoder_output_sizes), reversed(self.encoder_input_sizes)))
        self.pred = ConvLayer(self.base_num_channels, self.num_output_channels, 1, activation=None, trainable=trainable)

    def check_size(self, h: int, w: int):
        """H and W multiples of 16 with whole groups of 4 pixels per image at the deepest level (the convolution kernels' rule; every
        shallower level then has them too): raises before anything is launched."""
        depth = 1 << self.num_encoders
        if h % depth != 0 or w % depth != 0 or h < depth or w < depth:
            raise ValueError(f"UNet needs H and W multiples of {depth} (got {h} x {w}): pad the events first")
        hl, wl = h // depth, w // depth
        if (hl * wl) % 4 != 0:
            raise ValueError(f"UNet at {h} x {w}: level {self.num_encoders} is {hl} x {wl} = {hl * wl} pixels per image, and the convolution "
                             "kernels need whole groups of 4 ((H/16) * (W/16) % 4 == 0)")

    def forward(self, x, event_scales=None):
        """x: [N, num_bins, H, W] float voxel grid (any layout) -> [N, num_output_channels, H, W] (contiguous, x's dtype; bfloat16 under
        autocast; float32 under training: the values of the bfloat16 kernel output widened exactly).  event_scales as in UNetRecurrent."""
        self.check_size(x.shape[-2], x.shape[-1])
        out_dtype = _out_dtype(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):      # the stem hands out bfloat16; every later layer keeps it
            x = self.encoders[0](x, scales=event_scales)
        blocks = [x]
        for encoder in self.encoders[1:]:
            x = encoder(x)
            blocks.append(x)
        for resblock in self.resblocks:
            x = resblock(x)
        for i, decoder in enumerate(self.decoders):
            x = decoder(x, blocks[self.num_encoders - i - 1], skip_type="concat")   # skip_concat + upsampling in one kernel (:350)
        flow = self.pred(x)                                     # no skip on the prediction (:352)
        if self.trainable and torch.is_grad_enabled():
            return flow.contiguous()                            # float32 (PredFn): the loss gradient reaches the backward kernel unrounded
        return flow.to(out_dtype, memory_format=torch.contiguous_format)


class EVFlowNet(nn.Module):
    """model/model.py:226-261: `unet` = UNet with EVFlowNet's hard-coded kwargs applied over what the YAML gives; stateless."""

    HARD_CODED = dict(base_num_channels=32, num_encoders=4, num_residual_blocks=2, num_output_channels=2, skip_type="concat", norm=None,
                      use_upsample_conv=True, kernel_size=3, channel_multiplier=2)        # model/model.py:234-245

    def __init__(self, unet_kwargs, trainable: bool = False):
        super().__init__()
        kw = dict(unet_kwargs)
        kw.update(self.HARD_CODED)
        self.num_bins = kw["num_bins"]
        self.num_encoders = kw["num_encoders"]
        self.trainable = bool(trainable)           # the YAML switch: model: {target: ..EVFlowNet, params: {unet_kwargs: .., trainable: true}}
        self.unet = UNet(kw, trainable=trainable)

    def reset_states(self):
        pass

    def forward(self, event_tensor, event_scales=None):
        """[N, num_bins, H, W] -> {'flow': [N,2,H,W] (x, y) displacement, 'image': 0 * flow[..., 0:1, :, :]} (model/model.py:259-261)."""
        flow = self.unet(event_tensor, event_scales)
        return {"flow": flow, "image": 0 * flow[..., 0:1, :, :]}

    def default_chunk(self, h: int, w: int) -> int:
        """Images per launch of forward_sequence: the largest tensor of an image is the last decoder's upsampled concat buffer,
        H x W x 4 * base_num_channels elements (128 per pixel), and the kernels index tensors below 2^31 elements -- 1023 images at 128 x 128."""
        return max(1, 0x7FFFFFFF // (h * w * 4 * self.unet.base_num_channels))

    def forward_sequence(self, events, event_scales=None, chunk=None):
        """The reference's time loop (model/train_flow_utils.py:343-352) as one call: events [N,T,num_bins,H,W] -> flow [N,T,2,H,W].  The
        network has no state, so the loop is the same network on N*T images: time is folded into the batch, `chunk` images per launch
        (default: default_chunk, from the kernels' 2^31-element limit).  Every convolution runs the kernel instance the per-step batch of
        N images gets (nhwc_ops.tile_like_batch), so the result equals the per-step loop bit for bit.  Inference only."""
        n, t_steps = _sequence_shape(events)
        if self.trainable and torch.is_grad_enabled():
            raise ValueError("forward_sequence is inference only: train with the per-step loop or forward() on a folded batch")
        self.unet.check_size(events.shape[-2], events.shape[-1])
        chunk = self.default_chunk(events.shape[-2], events.shape[-1]) if chunk is None else max(1, int(chunk))
        ev = events.reshape((n * t_steps,) + tuple(events.shape[2:]))                  # n-major: image i = (i // T, i % T); a view when contiguous
        sc = event_scales.repeat_interleave(t_steps, dim=0) if event_scales is not None else None
        flows = []
        with torch.no_grad(), tile_like_batch(n):
            for i in range(0, n * t_steps, chunk):
                flows.append(self.unet(ev[i:i + chunk], None if sc is None else sc[i:i + chunk]))
        flow = flows[0] if len(flows) == 1 else torch.cat(flows)
        return flow.reshape((n, t_steps) + tuple(flow.shape[1:]))
