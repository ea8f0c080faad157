"""Frame pipelining of the tracker: which stream a frame's work goes on, and who waits for whom.

Opt-in through ``Ramp_vo.inputs_ready``: the caller guarantees that the tensors it hands to ``__call__`` are complete (not
still being produced on the current stream).  In the device-resident steady state the next frame's front end is then launched
on a side stream, gated by an event recorded before the last kernel of the previous frame's update operator: it runs next to
the gru chain and BA (a few small blocks on a 256-CU chip).
inputs_ready = "stream": the same pipelining for callers whose tensors ARE still being produced on the current stream when
they call (the reference's evaluate.py resizes each frame right before slam(...)): the tracker records an event on the
caller's stream, its front end waits for THAT, and everything else of the tracker runs on the tracker's own stream
(main_stream) -- so the caller's stream carries the caller's work only and the next frame's inputs are not queued behind this
frame's bundle adjustment.  The caller's stream in turn waits until the front end has taken its copy of the inputs (they may
be overwritten or freed right after the call, as on one stream).  Same contract for reading state as with True: through
settle() / update() / terminate() / peek() / state_dict() / the n, m, ii ... properties, which join the tracker's stream
first.  rampvo_amd.evaluate.run sets it.  RAMP_INPUTS_READY=stream|1 sets the default without touching the caller's code (the
reference's evaluate.py with its imports redirected: it reads points_ / colors_ / m only behind its closing update() calls,
which join).

What makes pipelined frames equal to sequential ones: a frame's front end reads the caller's inputs and the encoder's own
state only, so it may start as early as the gate lets it (the gate orders timing, never data); the frame commit reads what the
front end wrote, so the step's stream waits for the front end's "done" (``fe_done_to``: data, a 20 s hang guard); and every
public entry point that runs on the caller's stream joins the tracker's streams first (``join_main``).
"""
import ctypes
import weakref

import torch

from . import _lib, track_dev

_FE_DELAY_US = 35          # the encoder graph held back behind the selection (fe_delay; 0 measured flat)
_GATE_FLAG_DELAY_US = 0
_FE_WAIT_PROBE = False      # (diagnostic, set by tools/fe_wait.py before the tracker is built: events around the main queue's wait for the front end)
# The front end's "done" is a data dependency (the frame commit reads fe_fmap1 / imap / gmap / patches): the wave that waits
# for its signal word must not give up while the producer can still arrive.  The time-out is a hang guard only -- 20 s, far
# beyond any profiler slow-down -- and a wait that does give up still raises sticky status bit 128, on which settle() /
# lazy_state() raise.  Runtimes that serialise kernels never get here (switches.Switches.flag_waits: events instead).  The gate
# wait (gate_wait) keeps its 50 ms: it orders nothing but timing (a front end that starts early is slower, not wrong).
_FE_DONE_TIMEOUT_US = 20000000

_LIVE = {}        # device index -> trackers alive on it (FramePipeline.flag_wait_is_safe)


def _live_dec(idx):
    _LIVE[idx] = _LIVE.get(idx, 1) - 1


class NoPipeline:
    """a tracker off the GPU (oracle.host_cpu.RampVoCPU, the tests' CPU twin) has no streams: nothing is queued aside, nothing waits"""
    main_used = gate_by_flag = False
    main_stream = cur_stream = None

    def on_caller_stream(self, frame):
        return frame()

    def join_main(self):
        pass

    def wait_input(self):
        pass


class FramePipeline:
    def __init__(self, dev, flag_waits):
        self.live_idx = idx = dev.index if dev.index is not None else torch.cuda.current_device()
        _LIVE[idx] = _LIVE.get(idx, 0) + 1
        weakref.finalize(self, _live_dec, idx)
        # cross-stream orders as signal words looked at by a sleeping wave (False: events -- RAMP_NO_FLAG_WAITS, or a
        # runtime that runs one kernel at a time, where the waiting wave would keep its producer off the GPU: ADVICE r4)
        self.device, self.flag_waits = dev, flag_waits
        self.fe_stream = torch.cuda.Stream(device=dev)
        self.main_stream = torch.cuda.Stream(device=dev)     # inputs_ready = "stream": the tracker's own main stream
        self.cur_stream = None            # the stream of the frame in flight (None between frames)
        self.main_used, self.user_dirty = False, True     # work queued on main_stream / tracker work on the caller's stream
        self.in_event_pending, self.taken_recorded = False, False
        self.ev_taken = torch.cuda.Event()
        # events are re-recorded every frame (creating one costs a hipEventCreate/Destroy pair per use)
        self.fe_done_sig, self.fe_done_seq = None, 0
        self.ev_fe_done, self.ev_gate, self.ev_in = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        for ev in (self.ev_fe_done, self.ev_gate, self.ev_in):
            ev.record()                      # torch creates the hipEvent lazily; csrc/track.hip records the raw handle
        self.gate_armed = False
        # the gate as a signal word the step stores a sequence number into (no event packet between the update
        # operator's launches: tools/mb/stream_signal.hip)
        self.gate_sig, self.gate_seq, self.gate_by_flag = None, 0, False
        self.fe_wait_pairs = []           # (_FE_WAIT_PROBE)

    # ------------------------------------------------------------------ one frame's bracket
    def on_caller_stream(self, frame):
        """everything of the frame on the caller's stream (inputs_ready False / True)"""
        self.join_main()
        self.cur_stream = torch.cuda.current_stream()
        try:
            return frame()
        finally:
            self.cur_stream = None

    def on_own_stream(self, input_, resident, frame):
        """inputs_ready = "stream": see above.  The caller's stream gets one event record and one event wait per frame."""
        user, main, fe = torch.cuda.current_stream(self.device), self.main_stream, self.fe_stream
        self.ev_in.record(user)                         # the inputs (and whatever else the caller enqueued) up to here
        for t in input_[:2]:
            if torch.is_tensor(t) and t.is_cuda:        # allocated on the caller's stream, read on the tracker's
                t.record_stream(main)
                t.record_stream(fe)
        # the main stream itself waits for the caller's stream only when it has to: after a public call ran tracker work
        # there (update(), settle() ...: join_main marks it), or when this frame's front end runs on the main stream (no
        # gate armed: host-driven frames, the first device-resident one) -- in the steady state the front-end stream's wait
        # is the only one, and the main stream keeps no event packet between two frames
        if self.user_dirty or not (resident and self.gate_armed):
            main.wait_event(self.ev_in)
            self.user_dirty = False
        self.in_event_pending, self.taken_recorded = True, False
        self.cur_stream = main
        try:
            with torch.cuda.stream(main):
                out = frame()
        finally:
            self.cur_stream = None
            self.in_event_pending = False
            self.main_used = True                       # (a settle() inside the call may have joined: there is new work now)
        # the caller may overwrite / free its tensors once the front end has run on them (a frame whose front end ran on the
        # tracker's main stream -- host-driven frames -- : once that frame is through)
        if not self.taken_recorded:
            self.ev_taken.record(main)
        user.wait_event(self.ev_taken)
        return out

    def join_main(self):
        """(public entry points that run on the caller's stream) everything the tracker enqueued on its own stream first"""
        self.user_dirty = True                        # (whatever follows runs tracker work on the caller's stream)
        if self.main_used:
            self.main_stream.synchronize()
            self.fe_stream.synchronize()
            self.main_used = False

    def cur(self):
        """the frame's stream; looked up once per __call__ (torch.cuda.current_stream() costs ~4 us)"""
        return self.cur_stream if self.cur_stream is not None else torch.cuda.current_stream()

    def wait_input(self):
        """inputs_ready = "stream", a host-driven frame's front end and intrinsics on the main stream: behind the caller's stream"""
        if self.in_event_pending:
            self.cur().wait_event(self.ev_in)

    # ------------------------------------------------------------------ the gate: previous step -> this front end
    def gate_signal(self):
        """the signal word of the gate, or None (no flag waits, no signal memory, or 2^31 frames behind us: the event
        then).  Where in the step the word is stored: csrc/track.hip (fp16: by the first SoftAgg launch)"""
        if self.gate_sig is None:
            with torch.cuda.device(self.device):          # (the word must live on the tracker's GPU, not the caller's current one)
                self.gate_sig = track_dev.Signal() if self.flag_waits else False
        sig = self.gate_sig
        return sig if (sig and sig.ptr is not None and self.gate_seq < 0x7FFFFFF0) else None

    def step_gate(self, inputs_ready):
        """the gate arguments of a one-call step (DeviceTrack.step): the word and its next number, else the event, else nothing"""
        sig = self.gate_signal() if inputs_ready else None
        if sig is not None:
            self.gate_seq += 1
        return dict(gate_event=self.ev_gate.cuda_event if (inputs_ready and sig is None) else None,
                    gate_flag=sig.ptr if sig is not None else None, gate_seq=self.gate_seq)

    def arm(self, inputs_ready, by_flag):
        """behind the step: the next frame's front end may run on its own stream, behind the gate that step carried"""
        self.gate_armed, self.gate_by_flag = inputs_ready, by_flag

    def gate_wait(self, fe, dv):
        """(front-end stream) wait for the previous frame's gate: the signal word if that step stored one, else the event"""
        if self.gate_by_flag:
            self.gate_sig.wait(fe, self.gate_seq, then_delay_us=_GATE_FLAG_DELAY_US, status=dv.status_ptr)
        else:
            fe.wait_event(self.ev_gate)

    def fe_delay(self):
        """(on the front-end stream, behind the selection) hold the encoder graph back a little: its LSTM launch should not
        arrive while the gru launch is still filling the chip (csrc/track.hip::trk_delay_kernel)"""
        if _FE_DELAY_US > 0:
            _lib.check(_lib.lib().ramp_stream_delay(_FE_DELAY_US, _lib.stream()), "ramp_stream_delay")

    def fe_done_to(self, fe, cur, dv, inputs_ready):
        """the front end's "done" for the main stream: a word in signal memory stored by a one-thread launch behind the
        encoder graph and looked at by one sleeping wave in front of the frame commit (no flag waits -- RAMP_NO_FLAG_WAITS,
        a runtime that serialises kernels -- or no signal memory: an event record + stream wait, ~10 us of
        packets on the serial chain even when the front end is long done).  The commit READS what the front end wrote, so
        this wait's time-out is a hang guard (20 s), not a scheduling choice"""
        if self.fe_done_sig is None:
            with torch.cuda.device(self.device):
                self.fe_done_sig = track_dev.Signal() if self.flag_waits else False
        sig = self.fe_done_sig
        # A spinning wave needs its producer to run CONCURRENTLY: the runtime maps streams onto a handful of hardware queues,
        # and a waiter that shares one with its producer would sit in front of it until the hang guard fires.  Two streams of
        # one tracker (the caller's + the front end's: inputs_ready = True) have been measured safe on every box; with a third
        # tracker stream (inputs_ready = "stream": main_stream), or a second tracker in the process, the DATA dependency goes
        # through an event -- the gate (gate_wait), which orders timing only, keeps its word
        if sig and self.flag_wait_is_safe(inputs_ready) and sig.ptr is not None and self.fe_done_seq < 0x7FFFFFF0:
            self.fe_done_seq += 1
            _lib.check(_lib.lib().ramp_stream_signal(ctypes.c_void_p(fe.cuda_stream), sig.ptr, self.fe_done_seq), "ramp_stream_signal")
            sig.wait(cur, self.fe_done_seq, timeout_us=_FE_DONE_TIMEOUT_US, status=dv.status_ptr)
        else:
            self.ev_fe_done.record(fe)
            cur.wait_event(self.ev_fe_done)

    def flag_wait_is_safe(self, inputs_ready):
        return inputs_ready is True and _LIVE.get(self.live_idx, 0) <= 1

    def front_end(self, dv, inputs_ready, patchify, ahead_of_gate=None):
        """a device-resident frame's front end on its own stream, next to what is left of the previous frame from the gru
        chain on (the caller's tensors are complete; the gate is recorded inside ramp_track_step).  patchify(pre_replay=...):
        the tracker's front-end call; ahead_of_gate(fe): what depends on the input alone, like the staging and the selection"""
        fe, cur = self.fe_stream, self.cur()
        # Where the encoder graph starts relative to the gru launch depends on that launch's tile (csrc/update_mlp.hip
        # picks 64 or 80 rows per workgroup by the factor count, tools/corun_gru_lstm.py): with 80-row tiles (two full
        # rounds of one workgroup per CU, 254 VGPRs) the front end's LSTM launch cannot take a CU from it, so the
        # selection goes out AHEAD of the gate and the graph right behind it; with 64-row tiles an LSTM launch that
        # arrives within ~40 us costs gru 45 us, so the selection runs behind the gate and the graph is held back
        # another 35 us (fe_delay).
        ahead = _lib.lib().ramp_upd_gru_tile_rows(dv.factor_estimate(), 0) == 80
        if self.in_event_pending:
            fe.wait_event(self.ev_in)               # inputs_ready = "stream": the caller's stream up to the call
        if ahead_of_gate is not None:
            ahead_of_gate(fe)                       # (behind the caller's stream, ahead of this frame's "done")
        if not ahead:
            self.gate_wait(fe, dv)
        with torch.cuda.stream(fe):
            out = patchify(pre_replay=(lambda: self.gate_wait(fe, dv)) if ahead else self.fe_delay)
        if self.in_event_pending:
            self.ev_taken.record(fe)
            self.taken_recorded = True
        if _FE_WAIT_PROBE:                      # (diagnostic: how long the main queue waits for the front end)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(cur)
            self.fe_done_to(fe, cur, dv, inputs_ready)
            b.record(cur)
            self.fe_wait_pairs.append((a, b))
        else:
            self.fe_done_to(fe, cur, dv, inputs_ready)
        if not dv.fp32:
            # (behind the event: the frame does not wait for it) the window's correlation planes back into the
            # memory-side cache while the previous frame's bundle adjustment is still running
            with torch.cuda.stream(fe):
                dv.warm()
        return out
