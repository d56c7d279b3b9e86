"""Lanes: consecutive wideband buffers on alternating HIP streams (no reference counterpart).

The reference's server handles one buffer at a time (examples/multi_fm_server.py:98-106: ``load``, then every channel's
``run`` -> ``demodulator.run``).  On the GPU every stage of that loop is a launch whose last workgroups leave part of the
chip idle, and the wideband FFT of buffer i + 1 does not depend on anything buffer i computes: with two handle sets
(spectrum + workspaces each), each on its own stream, the kernels of the next buffer fill the gaps of the current one.
The ONE thing buffer i + 1 needs from buffer i is the de-emphasis state (deemphasis.py:64; mfm.py:63, wbfm.py:97-100):
the lanes share it, and librcfm orders the launches that touch it across streams (RCFM_OPT_STATE_FENCE), so the audio is
bit-identical to the one-buffer-at-a-time loop.

Measured (`pipelined` blocks of profiles/r04_i_bench.json, same box as the one-lane figure): cfg4 -2 %, cfg5 -2 %, cfg3 (64 channels, launches of a few
tiles per CU) -11 %.  Costs one more spectrum and workspace set per lane (cfg4: 14 GB).
"""

from collections import namedtuple

from radiocore._internal import hip
from radiocore.tools.tuner import Tuner

__all__ = ["Lanes"]


# One submitted buffer until result() collects it: the event behind its last launch, the event behind its load (= the last
# reader of the input), the Tuner's run record (audio blocks, squelch masks or None, tone powers or None), submit's `each`.
_Pending = namedtuple("_Pending", "end loaded run each")


class Lanes:
    """``depth`` buffers in flight through one Tuner's channels.

        lanes = Lanes(tuner, depth=2)
        t0 = lanes.submit(buffer0)          # returns at once; load + run_all are queued on lane 0's stream
        t1 = lanes.submit(buffer1)          # lane 1: overlaps buffer0's kernels
        audio0 = lanes.result(t0)           # [C, A, ch] like Tuner.run_all(); waits for that buffer only

    Buffers are demodulated in submission order as far as the per-channel state is concerned; results may be collected
    in any order, each once.  ``tuner`` stays usable on its own between submissions (it is lane 0).
    Submit from ONE host thread (or order the calls yourself): the order of the host calls is the order of the buffers,
    and the fence is armed by whichever call came last.  Before resetting or reading a demodulator's state by hand
    (``demodulator.reset()``), ``drain()`` first.
    """

    def __init__(self, tuner: Tuner, depth: int = 2, timing: bool = False):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self._torch = hip.torch()
        self._timing = bool(timing)     # events that can be timed: overlap_ms() (tests, tuning), not needed otherwise
        self._base = tuner
        tuner._arm_state_fence()
        self._tuners = [tuner] + [tuner._lane_clone() for _ in range(depth - 1)]
        self._streams = [self._torch.cuda.Stream() for _ in range(depth)]
        self._next = 0
        self._pending = {}          # ticket -> _Pending
        self._spans = {}            # timing=True: ticket -> (start event, end event)

    @property
    def depth(self) -> int:
        return len(self._tuners)

    def submit(self, input_signal, chunk: int = 0, each: bool = False, raw: bool = False) -> int:
        """Queue Tuner.load + Tuner.run_all of one buffer on the next lane; returns a ticket for ``result``.
        each=True: Tuner.run_each instead (channels of different classes and geometries; ``result`` then returns its
        list of per-channel arrays).  With ``tuner.set_squelch`` set, the lane queues the levels and the squelch behind
        its demodulators like ``run_all`` does; ``result(ticket, open_mask=True)`` returns the buffer's mask.  The same
        holds for ``tuner.set_tones``: ``result(ticket, tones=True)`` returns the buffer's tone powers.
        raw=True: ``input_signal`` holds interleaved integer I, Q and the lane loads it with Tuner.load_raw."""
        ticket = self._next
        self._next += 1
        k = ticket % len(self._tuners)
        t = self._tuners[k]
        if k:
            t._sync_lane(self._base)            # channels added since the lane was made
        st = self._streams[k]
        st.wait_stream(self._torch.cuda.current_stream())     # whatever produced the buffer
        if isinstance(input_signal, self._torch.Tensor) and input_signal.is_cuda:
            # the caller's tensor is read on the lane's stream: the caching allocator must not hand its memory to
            # current-stream work before the lane's FFT has consumed it
            input_signal.record_stream(st)
        with self._torch.cuda.stream(st):
            start = self._event(st) if self._timing else None
            (t.load_raw if raw else t.load)(input_signal)
            loaded = self._event(st)            # the wideband FFT is the LAST reader of the input buffer
            run = t._run_each_device() if each else t._run_all_device(chunk)
            ev = self._event(st)
        self._pending[ticket] = _Pending(ev, loaded, run, each)
        if self._timing:
            self._spans[ticket] = (start, ev)
        return ticket

    def _event(self, stream):
        e = self._torch.cuda.Event(enable_timing=self._timing)
        e.record(stream)
        return e

    def overlap_ms(self, earlier: int, later: int) -> float:
        """timing=True only: how long before the END of buffer `earlier` the lane of buffer `later` started working
        (positive: the two buffers overlapped on the device; negative: `later` started that long after `earlier` had
        finished).  Both must have completed (result() / drain())."""
        start, _ = self._spans[later]
        _, end = self._spans[earlier]
        return float(start.elapsed_time(end))

    def result(self, ticket: int, numpy_output: bool = True, open_mask: bool = False, tones: bool = False,
               frame_mask: bool = False, mix: bool = False):
        """The audio of one submitted buffer, [C, A, ch] float32 (the shard's block after Tuner.shard).
        open_mask=True: ``(audio, mask)`` with the squelch's numpy bool [C] of that buffer (Tuner.open_mask; None when
        the buffer was submitted with squelch off).  frame_mask=True: the frame gate's numpy bool [C, frames] of that
        buffer follows (Tuner.frame_mask; None when it was submitted without a gate).  tones=True: the tone bank's
        ``(P, E)`` of that buffer (Tuner.tone_power; None when it was submitted without a bank) follows.  mix=True: the
        buffer's buses (Tuner.mix; None when it was submitted without a mixer) come last in the tuple."""
        entry = self._pending.pop(ticket)
        run = entry.run
        device_output = self._base._cuda and not numpy_output
        if device_output:
            cur = self._torch.cuda.current_stream()
            cur.wait_event(entry.end)                          # stream-ordered hand-over, no host wait
            for _, _, a in run.blocks:
                a.record_stream(cur)
        else:
            entry.end.synchronize()
        out = self._base._each_result(run.blocks, device_output) if entry.each else \
            self._base._result(run.blocks[0][2], device_output)
        extra = []
        if open_mask:
            extra.append(Tuner._mask_result(run.masks) if run.masks is not None else None)
        if frame_mask:
            extra.append(Tuner._frame_result(run.frames) if run.frames is not None else None)
        if tones:
            if device_output and run.tones is not None:
                for p, e in run.tones:
                    p.record_stream(cur)
                    e.record_stream(cur)
            extra.append(self._base._tone_result(run.tones, device_output) if run.tones is not None else None)
        if mix:
            if device_output and run.mix is not None:
                for o, _, _ in run.mix[1]:
                    o.record_stream(cur)
            extra.append(self._base._mix_result(run.mix, device_output) if run.mix is not None else None)
        return (out, *extra) if extra else out

    def hold_current_stream(self, ticket: int):
        """Order the CURRENT stream behind the last READ of one submitted buffer's input (the wideband FFT of
        Tuner.load; the channel stages read the spectrum, not the input): for a caller that recycles the buffer's
        storage stream-ordered (``with feeder.next() as x: t = lanes.submit(x); lanes.hold_current_stream(t)`` -- the
        Feeder frees the slot behind the current stream, which must therefore wait for the lane that still reads it).
        It does NOT wait for the buffer's audio: the next submit() waits for the current stream, and a wait for the
        whole buffer there would run the lanes one after the other.
        Caveat: streams share in-order hardware queues when the runtime has fewer queues than streams (GPU_MAX_HW_QUEUES;
        with 2, the default stream shares one with a lane).  The current stream's wait then lasts until everything
        queued before it on that queue has run -- the lane's whole buffer -- and the lanes serialise.  On such a runtime,
        run the recipe from a stream that gets a queue of its own, e.g. ``torch.cuda.Stream(priority=-1)`` (each
        priority has its own queues) made current in a process whose streams do not already fill that priority's
        queues (tests/test_hip_lanes.py)."""
        self._torch.cuda.current_stream().wait_event(self._pending[ticket].loaded)

    def drain(self):
        """Wait for everything submitted so far (results stay collectable)."""
        for entry in self._pending.values():
            entry.end.synchronize()
