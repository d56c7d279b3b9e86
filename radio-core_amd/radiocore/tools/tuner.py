"""Tuner: FFT channelizer (reference: radiocore/tools/tuner.py:9-174).

Channel bookkeeping stays host-side Python with the reference's arithmetic; the
wideband FFT, the per-channel bin gather / weight / inverse FFT and (for
``run_all``) the demodulators run in librcfm.so.
"""

import ctypes
from collections import namedtuple
from dataclasses import dataclass
from typing import List

import numpy as np

from radiocore._internal import Injector, hip
from radiocore.tools import busdyn, iq, spectrum
from radiocore.tools.floor import OverFloor, channel_noise_gain

__all__ = ["Tuner", "Channel"]

_KINDS = {"FM": hip.RCFM_FM, "MFM": hip.RCFM_MFM, "WBFM": hip.RCFM_WBFM, "AM": hip.RCFM_AM,
          "USB": hip.RCFM_USB, "LSB": hip.RCFM_LSB}
_STATELESS = (hip.RCFM_FM, hip.RCFM_AM, hip.RCFM_USB, hip.RCFM_LSB)    # kinds without de-emphasis state: nothing to bind or fence
                                                                       # (unless AM / USB / LSB carry an AGC: its state is bound and fenced)
_DEFAULT_OPTIONS = (True, True, True, 1, True)                         # set_kernel_options: lds_chain, fused_tiles, phase_link, narrow_tiles, ssb_direct
# What one run_all / run_each queued, on the device, one entry per launch group: blocks [(n, ch, audio [n, A, ch])]; masks, the
# squelch's uint8 [n], or None (no squelch was set, or nothing was gated); tones, the bank's (P, E), or None (no bank was set);
# frames, the frame gate's uint8 [n, F + 1], or None (no gate was set).  mix, not per group: None (no mixer was set) or
# (owner [M], the group each bus belongs to, [(out [M, A, ch_out], active int32 [M], bus_open uint8 [M]) per group]).  dry: None
# (no bus dynamics were set) or what the mixer itself wrote, in the form of mix -- whose rows and bus_open then are the
# processed ones -- with the block length L as a fourth entry per group.
_Run = namedtuple("_Run", "blocks masks tones frames mix dry", defaults=(None, None, None, None, None, None))
_FRAME_SCRATCH_BYTES = 256 << 20                                       # frame_levels: the most channel IQ held at a time


class _Part:
    """Elements [first, first + count) of a float32 device tensor, where a whole tensor of thresholds is expected."""

    def __init__(self, whole, first, count):
        self._whole, self._first, self._count = whole, first, count

    def data_ptr(self):
        return self._whole.data_ptr() + 4 * self._first

    def tensor(self):
        return self._whole[self._first:self._first + self._count]


class _Carried(dict):
    """One cache of librcfm handles whose device state is carried from buffer to buffer and shared with the lanes (DESIGN.md,
    "carried state"): a dict with the entry layout its stage chose, which knows where the hip.Handles sit in an entry and
    which ABI functions put such a handle's state back to rest and arm its fence (None: it has none).  The Tuner walks
    them in one ordered collection (``_carried``) and stores with ``put``, which arms a handle made after the lanes were."""

    def __init__(self, handles_of, reset=None, fence=None):
        super().__init__()
        self._handles_of, self._reset, self._fence = handles_of, reset, fence

    def _each(self, name, entries, arg):
        if name is not None:
            for h in [h for e in entries for h in self._handles_of(e)]:
                hip.check(getattr(hip.lib(), name)(h.value, arg))

    def reset_states(self):
        self._each(self._reset, self.values(), hip.stream())

    def arm(self):
        self._each(self._fence, self.values(), 1)

    def put(self, key, entry, fenced):
        self._each(self._fence, (entry,) if fenced else (), 1)
        self[key] = entry
        return entry


# _sync_lane: the settings a lane follows -> what of the lane's own a new one drops (None: it is made again when next used, _derived)
_FOLLOWED = {"_squelch": "last", "_tones": "last", "_gate": "last", "_mix": "last", "_busdyn": "last", "_blanker": "blanker",
             "_floor": "floor", "_afilt": None, "_iq_balance": None, "_fine": None}


def _key_agc(key):
    """The AGC setting (decay_samples, level, floor) a _batched key ends with, or None."""
    last = key[-1]
    return last[1] if isinstance(last, tuple) and last[:1] == ("agc",) else None


@dataclass
class Channel:
    """Frequency boundaries of one channel plus its demodulator (tuner.py:9-36)."""

    index: int
    bandwidth: float
    demodulator: None
    lower_frequency: float
    center_frequency: float
    higher_frequency: float

    @property
    def address_bytes(self) -> bytes:
        return int(self.center_frequency).to_bytes(4, byteorder='little')


class Tuner(Injector):
    """Channelizes one-second wideband buffers.

    Reference-compatible use: add_channel / request_bandwidth / load / run(i).
    Batched use (this build): ``run_all()`` after ``load`` returns the audio of
    every channel in one call -- the loop of examples/multi_fm_server.py:100-106.
    """

    def __init__(self, cuda: bool = False):
        self._cuda = cuda
        super().__init__(self._cuda)
        self._arena = hip.current_arena()     # `with radiocore.tools.Arena(...)`: the device handles are built inside it
        self._input_frequency = 0.0
        self._input_bandwidth = 0.0
        self._bounds: List[Channel] = []
        self._handle = None        # librcfm tuner, rebuilt when the geometry changes
        self._handle_key = None
        self._shard = None         # (first, count) declared by shard()
        self._loaded_size = None
        self._win_size = None      # length of the reference's cached window (set by the first run)
        self._batched = {}         # (kind, C, B, A, tau, chunk) -> demod handle of run_all / run_each
        # Everything below is derived from the channel list and rebuilt only when add_channel / reset change it
        # (`_version`): load / run / run_all do no per-channel Python work in the steady state.
        self._version = 0
        self._lo = self._hi = self._bw_sum = None     # running min / max / sum of _recalculate
        self._abi_arrays = None    # (version, rolls, bws, the _fine the rolls include) as ctypes arrays
        self._plan = None          # (version, shard) -> run_all / run_each launch plan
        self._uniform = (None, None)   # (version, the one geometry all channels share or None)
        self._state_owner = {}     # (kind, C, B, A, tau) -> the batched handle whose buffer holds that geometry's state
        self._bound_version = {}   # batched key -> channel-list version its demodulators were bound at
        self._state_fence = False  # Lanes: this tuner's batched handles run on several streams (RCFM_OPT_STATE_FENCE)
        self._is_lane = False      # _lane_clone: a second device tuner over another Tuner's channels and states
        self._kernel_options = _DEFAULT_OPTIONS
        self._taps = {}            # (B, R, f, taps) -> (channels it holds, batched subcarrier handle) of subcarrier()
        # The settings: host values, replaced by their set_* and never changed in place, so that a lane follows by identity.
        self._squelch = None       # set_squelch: None (off), float32 thresholds, 0-d (every channel) or [len(channels())], or an OverFloor
        self._fine = None          # retune: None or int64 [len(channels())] bins each channel was moved up
        self._iq_balance = None    # set_iq_balance: None (off) or (mode, beta, dc_notch)
        self._tones = None         # set_tones: None (off) or (bank, want int32 [C] or None, ratio float32 [C] or None)
        self._afilt = None         # set_audio_filter: None (off) or (AudioFilter, uint8 [C] or None)
        self._blanker = None       # set_blanker: None (off) or (NoiseBlanker, in_place)
        self._gate = None          # set_gate: None (off) or (FrameGate, open float32, close float32: 0-d or [len(channels())]; or two OverFloor)
        self._floor = None         # set_floor: None (off) or the NoiseFloor
        self._mix = None           # set_mix: None (off) or the Mixer
        self._busdyn = None        # set_bus_dynamics: None (off) or (Limiter, {bus: Duck} or None)
        # What is made FROM a setting -- device copies, "fits this launch plan", what the device handle was last told -- is
        # looked up with what it is made from (_derived) and made again when that differs: nothing invalidates it by hand.
        self._built = {}           # name -> (setting, channel-list version / launch-plan key / handle key, what was made)
        self._last = _Run()        # masks and tone powers of the last run_all / run_each (not its audio: the caller's)
        # Device state that is no copy of a setting.  What is carried from buffer to buffer: one cache per stage, each also the attribute of
        # its name, in the order reset_states() and _arm_state_fence() walk; reset() empties them, a lane shares them.  A new stage adds ONE entry.
        self._carried = {
            "_afilt_handles": _Carried(lambda e: e[2:], "rcfm_audio_filter_reset", "rcfm_audio_filter_set_fence"),   # (legs, A) -> (channels, AudioFilter, librcfm handle): the filter's states, by channel index
            "_gate_handles": _Carried(lambda e: e[2:], "rcfm_gate_reset", "rcfm_gate_set_fence"),   # A -> (channels, FrameGate, librcfm handle): the gate's states, by channel index
            "_floor_handles": _Carried(lambda e: e[1:], "rcfm_floor_reset", "rcfm_floor_set_fence"),   # buffer length n -> (NoiseFloor, librcfm handle): the tracked floor
            "_mix_handles": _Carried(lambda e: e[3]),   # the launch groups ((first, count), ..) -> (Mixer, channel-list version, owner [M], librcfm handle per group): no state
            "_busdyn_handles": _Carried(lambda e: [h for _, h in e[1]], "rcfm_busdyn_reset", "rcfm_busdyn_set_fence"),   # (M, ch_out, the groups' audio lengths) -> ((Limiter, ducks), [(L, librcfm handle) per group]): the limiter's state
        }
        self.__dict__.update(self._carried)
        self._floor_out = None     # the last load with a floor set: (n, cells, power, floor, {db: thresholds [C]}) on the device, each lane's own
        self._frame_scratch = None # frame_levels: the channel IQ of a chunk, this device tuner's own (allocated by the first call, kept)
        self._blank_handles = {}   # buffer length n -> (the NoiseBlanker it was made by, librcfm handle): this device tuner's own scratch
        self._blank_scratch = None # the blanked copy of a caller's device tensor (buffer's dtype and size; allocated by the first such load)
        self._blank_counts = None  # device int64 [2] of the last load with a blanker: hits, samples with gain below 1

    @property
    def input_frequency(self) -> float:
        """Return the center frequency of the input data."""
        return self._input_frequency

    @property
    def input_bandwidth(self) -> float:
        """Return the bandwidth of the input data."""
        return self._input_bandwidth

    def channels(self) -> List[Channel]:
        """Return list of registered channels."""
        return self._bounds

    def request_bandwidth(self, bandwidth: float):
        """Override the calculated bandwidth (must not be below it)."""
        if bandwidth < self._input_bandwidth:
            raise ValueError(f"requested bandwidth ({bandwidth}) is too low, "
                             f"minimum is {self._input_bandwidth}")
        self._input_bandwidth = bandwidth

    def add_channel(self, frequency: float, bandwidth: float, demodulator):
        """Register a channel; recalculates the input geometry."""
        ch = Channel(
            index=len(self._bounds),
            bandwidth=bandwidth,
            demodulator=demodulator,
            lower_frequency=(frequency - (bandwidth / 2)),
            center_frequency=frequency,
            higher_frequency=(frequency + (bandwidth / 2)),
        )
        self._bounds.append(ch)
        self._recalculate(ch)

    def reset(self):
        """Forget all channels (raises ValueError like the reference: min() of nothing)."""
        self._bounds = []
        self._lo = self._hi = self._bw_sum = None
        for cache in self._carried.values():
            cache.clear()                  # the carried states belong to the channels, the tracked floor to their band
        self._floor_out = None
        self._recalculate()

    def _recalculate(self, added=None):
        # tuner.py:163-174.  The reference recomputes min / max / sum over every channel on each add_channel (O(C^2)
        # to set up C channels: 2.9 s for 8192); the running forms below give the same floats in O(1) per channel: min
        # and max are exact, and the running total equals sum() whenever the bandwidths are integer-valued floats below
        # 2^53 (every partial sum is exact) -- the only bandwidths with a meaning here, since int(bandwidth) is the
        # channel's sample count (tuner.py:153).  For non-integer bandwidths Python >= 3.12's compensated sum() may
        # differ from the running total in the last bit.  Channel objects are not expected to change after add_channel
        # (the device handle is keyed by the list's version, not by its contents).
        self._version += 1
        self._fine = None          # the fine-tune belongs to the channel list's version
        if added is not None and self._lo is not None:
            self._lo = min(self._lo, added.lower_frequency)
            self._hi = max(self._hi, added.higher_frequency)
            self._bw_sum = self._bw_sum + added.bandwidth
        else:
            self._lo = min([ch.lower_frequency for ch in self._bounds])
            self._hi = max([ch.higher_frequency for ch in self._bounds])
            self._bw_sum = sum([ch.bandwidth for ch in self._bounds])
        lower, higher = self._lo, self._hi
        self._input_frequency = (lower + higher) / 2
        self._input_bandwidth = (higher - lower)
        mean_bandwidth = self._bw_sum
        mean_bandwidth //= len(self._bounds)
        self._input_bandwidth += (self._input_bandwidth * -1) % mean_bandwidth

    def _derived(self, name, setting, key, make):
        """What `make()` made for `name` from `setting` (compared by identity) under `key` (channel-list version, launch-plan
        key or device handle's key, compared by value): made now unless just that is held.  A `make` that raises keeps nothing."""
        held = self._built.get(name)
        if held is None or held[0] is not setting or held[1] != key:
            held = self._built[name] = (setting, key, make())
        return held[2]

    def _per_channel(self, a, what, scalar=True):
        """The array `a` -- one value per channel, or (scalar=True) one for all -- or ValueError: `what` and the count."""
        C = len(self._bounds)
        if a.ndim > 1 or (a.ndim == 0 and not scalar) or (a.ndim == 1 and a.shape[0] != C):
            raise ValueError("%s (%d)" % (what, C))
        return a

    def _out(self, tensor, numpy_output):
        """A device tensor as the caller asked for it: left on the device only by a cuda=True tuner with numpy_output=False."""
        return self._result(tensor, self._cuda and not numpy_output)

    # ---- device side ---------------------------------------------------------

    def _device_tuner(self, n):
        # rolls depend on the channel list only (input_frequency is recomputed by add_channel, never by
        # request_bandwidth) and on the fine-tune: the handle is keyed by (n, _version) and the O(C) lists are built once
        # per version and retune
        key = (n, self._version)
        if key != self._handle_key:
            held = self._abi_arrays
            if held is None or held[0] != self._version or held[3] is not self._fine:
                bws = [int(ch.bandwidth) for ch in self._bounds]
                held = self._abi_arrays = (self._version, self._rolls(self._fine), (ctypes.c_int32 * len(bws))(*bws), self._fine)
            h = ctypes.c_void_p()
            with hip.bound(self._arena):
                hip.check(self._lib.rcfm_tuner_create(n, len(self._bounds), held[1], held[2], ctypes.byref(h)))
            self._handle = hip.Handle(h, self._lib.rcfm_tuner_destroy)
            self._handle_key = key
            self._loaded_size = None
            self._built["fine"] = (self._fine, key, None)      # what a new handle knows: the rolls it was made with ...
            self._built["iq"] = (None, key, None)              # ... and no IQ balance
            if self._shard is not None:
                hip.check(self._lib.rcfm_tuner_shard(h, self._shard[0], self._shard[1]))
            self._follow(h)
        return self._handle.value

    def _follow(self, h):
        # the device handle h is told of a retune and a set_iq_balance it has not seen (one that exists is told by those calls
        # themselves): a new handle, and a lane's with the lane's next load, on its own stream (per buffer, nothing to fence)
        self._derived("fine", self._fine, self._handle_key, lambda: self._retune(h, self._fine))
        self._derived("iq", self._iq_balance, self._handle_key, lambda: self._apply_iq_balance(h))

    def _rolls(self, fine):
        # roll[c] = int(f_in - f_c) (tuner.py:152) minus the bins the channel was moved up by retune
        rolls = [int(self._input_frequency - ch.center_frequency) for ch in self._bounds]
        if fine is not None:
            rolls = [r - int(k) for r, k in zip(rolls, fine)]
        return (ctypes.c_int64 * len(rolls))(*rolls)

    def _retune(self, handle, fine):
        hip.check(self._lib.rcfm_tuner_retune(handle, 0, len(self._bounds), self._rolls(fine), hip.stream()))

    def shard(self, first, count):
        """Multi-GPU only (no reference counterpart): this process will run channels
        [first, first + count) and nothing else, so `load` may keep just the part of the spectrum
        they read (sharding.channel_range gives the range of a rank)."""
        if first < 0 or count < 0 or first + count > len(self._bounds):
            raise IndexError("channel range outside the tuner")
        self._shard = (int(first), int(count))
        if self._handle is not None:
            hip.check(self._lib.rcfm_tuner_shard(self._handle.value, int(first), int(count)))

    def load(self, input_signal, whole=False):
        """Forward FFT of the one-second buffer; kept on the device (tuner.py:126-138).

        whole=True (multi-GPU, rotating FFT owner): keep every row any channel reads although this process is
        sharded -- the spectrum is about to be handed to the other ranks (sharding.SpectrumRing)."""
        x = hip.to_device(input_signal, self._torch.complex64)
        self._load(x, int(x.shape[0]), whole, lambda h, src: self._lib.rcfm_tuner_load(h, hip.ptr(src), hip.stream()),
                   hip.RCFM_IQ_CF32, input_signal)

    def load_raw(self, samples, whole=False):
        """``load`` of a buffer as the receiver delivers it (rcfm_tuner_load_raw; no reference counterpart): a numpy array
        or torch tensor of interleaved I, Q integers, [N, 2] or [2 N], whose dtype names the format -- int16 (Airspy, USRP
        wire format), int8 (HackRF) or uint8 (RTL-SDR, centre 127.5) -- full scale 1.0.  The spectrum, and so everything run
        from it, is bit for bit that of ``load(iq.to_complex64(samples))``; the buffer crosses PCIe and is read by the
        wideband FFT at 4 or 2 bytes per sample instead of 8, and no complex64 copy of it is made.  ValueError for any other
        dtype, an odd element count, or an N that is not the tuner's input size."""
        x, fmt, n = iq.device_pairs(samples)
        if n != int(self._input_bandwidth):
            raise ValueError("input_sig size and input_size mismatch")
        self._load(x, n, whole, lambda h, src: self._lib.rcfm_tuner_load_raw(h, fmt, hip.ptr(src), hip.stream()),
                   fmt, samples)

    def _is_upload(self, given, x):
        # True when the device buffer x is a tensor made for this load (a host array's upload, a converted copy), not the
        # caller's own device tensor
        return not (isinstance(given, self._torch.Tensor) and given.is_cuda and given.data_ptr() == x.data_ptr())

    def _load(self, x, n, whole, call, fmt, given):
        # what load and load_raw share: `call(handle, buffer)` is the library's load of a device buffer of n samples -- x,
        # or what the blanker made of it
        if self._floor is not None:
            self._floor_whole("load")
        h = self._device_tuner(n)
        if self._blanker is not None:
            x = self._blank(x, n, fmt, self._is_upload(given, x))
        self._follow(h)
        if whole and self._shard is not None:
            hip.check(self._lib.rcfm_tuner_shard(h, 0, len(self._bounds)))
            try:
                hip.check(call(h, x))
            finally:      # a failed load must not leave the handle sharded to every channel
                hip.check(self._lib.rcfm_tuner_shard(h, self._shard[0], self._shard[1]))
        else:
            hip.check(call(h, x))
        self._input = x            # keeps the buffer alive until the FFT has consumed it
        self._loaded_size = n
        self._floor_out = None
        if self._floor is not None:
            self._floor_pass(h, n)

    # ---- the spectrum as an object that can travel (rcfm_tuner_attach_spectrum / _window / _adopt) ---------------

    def spectrum_slot(self, n):
        """Device storage for one spectrum of an n-sample buffer: complex64 [halo + n + halo] (torch owns it)."""
        halo, nn = ctypes.c_int64(), ctypes.c_int64()
        hip.check(self._lib.rcfm_tuner_spectrum_layout(self._device_tuner(int(n)), ctypes.byref(halo), ctypes.byref(nn)))
        t = hip.empty((int(nn.value) + 2 * int(halo.value),), self._torch.complex64)
        t.rcfm_halo = int(halo.value)
        return t

    def _same_handle(self, n, what):
        """The device handle for length n -- refusing to REBUILD it: a handle of another length would silently drop the
        attached spectrum and the loaded state (the handle is keyed by (n, channel-list version))."""
        if self._handle is not None and self._handle_key is not None and self._handle_key[0] != int(n) and \
                self._handle_key[1] == self._version:
            raise ValueError("%s: this tuner's device handle was built for %d-sample buffers, not %d"
                             % (what, self._handle_key[0], int(n)))
        return self._device_tuner(int(n))

    def attach(self, slot, n, loaded=None):
        """Use `slot` (from spectrum_slot) as the spectrum from now on; loaded = (first, count): it already holds the
        bins those channels read (None: nothing yet -- a load or adopt must follow)."""
        first, count = loaded if loaded is not None else (0, 0)
        hip.check(self._lib.rcfm_tuner_attach_spectrum(self._same_handle(n, "attach"), hip.ptr(slot), int(first), int(count)))
        self._slot = slot          # keeps the storage alive while the handle points at it
        self._loaded_size = int(n) if loaded is not None else None

    def detach(self, n):
        """Back to the handle's own spectrum storage (nothing loaded)."""
        hip.check(self._lib.rcfm_tuner_attach_spectrum(self._same_handle(n, "detach"), None, 0, 0))
        self._slot = None
        self._loaded_size = None

    def window_slot(self, n, first, count):
        """Device storage for just the bins channels [first, first + count) read -- complex64 [halo + nbins + halo], the
        window's first bin at element `halo` -- or None when that window wraps around the ends of the spectrum (such a
        range needs a whole spectrum_slot).  What a rank that never owns a buffer keeps per buffer in flight."""
        halo, nb = ctypes.c_int64(), ctypes.c_int64()
        rc = self._lib.rcfm_tuner_window_layout(self._device_tuner(int(n)), int(first), int(count), ctypes.byref(halo),
                                                ctypes.byref(nb))
        if rc != 0:
            return None
        t = hip.empty((int(nb.value) + 2 * int(halo.value),), self._torch.complex64)
        t.rcfm_halo = int(halo.value)
        t.rcfm_window = (int(first), int(count))
        return t

    def attach_window(self, slot, n):
        """Use `slot` (from window_slot) as the spectrum of its channel range; adopt() must follow once the bins are in."""
        first, count = slot.rcfm_window
        hip.check(self._lib.rcfm_tuner_attach_window(self._same_handle(n, "attach_window"), hip.ptr(slot), first, count))
        self._slot = slot
        self._loaded_size = None

    def window(self, n, first, count):
        """(first_bin, nbins): the bins of an n-point spectrum that channels [first, first + count) read, modulo n."""
        fb, nb = ctypes.c_int64(), ctypes.c_int64()
        hip.check(self._lib.rcfm_tuner_window(self._device_tuner(int(n)), int(first), int(count), ctypes.byref(fb),
                                              ctypes.byref(nb)))
        return int(fb.value), int(nb.value)

    def adopt(self, n, first, count):
        """The caller has written window(n, first, count) into the attached slot: accept it as loaded."""
        hip.check(self._lib.rcfm_tuner_adopt(self._same_handle(n, "adopt"), int(first), int(count), hip.stream()))
        self._loaded_size = int(n)

    def _ready(self):
        if self._loaded_size is None:
            raise RuntimeError("Tuner.run called before Tuner.load")
        # tuner.py:155-157 builds the spectral window on the first run() with int(input_bandwidth) points and never
        # refreshes it; scipy.signal.resample then refuses any buffer of another length -- also after a later
        # request_bandwidth().  Same behaviour here: the first run fixes the size.
        if self._win_size is None:
            self._win_size = int(self._input_bandwidth)
        if self._loaded_size != self._win_size:
            raise ValueError('window must have the same length as data')
        return self._device_tuner(self._loaded_size)

    def run(self, channel_index: int):
        """Channelized complex64 signal of one channel (tuner.py:140-161)."""
        channel = self._bounds[int(channel_index)]
        handle = self._ready()
        out = hip.empty((int(channel.bandwidth),), self._torch.complex64)
        hip.check(self._lib.rcfm_tuner_run(handle, int(channel_index), 1, hip.ptr(out), hip.stream()))
        return self._result(out, self._cuda)

    def run_channels(self, first: int, count: int):
        """[count, B] complex64 device tensor for a range of equal-bandwidth channels."""
        handle = self._ready()
        if count <= 0 or first < 0 or first + count > len(self._bounds):
            raise IndexError("list index out of range")
        out = hip.empty((count, int(self._bounds[first].bandwidth)), self._torch.complex64)
        hip.check(self._lib.rcfm_tuner_run(handle, first, count, hip.ptr(out), hip.stream()))
        return out

    # ---- signal levels and squelch (rcfm_tuner_levels / rcfm_squelch; no reference counterpart) ----------------------

    def levels(self, numpy_output: bool = True):
        """Signal level of every channel (of the shard's range after ``shard``), float32 [count]: the mean power
        ``mean(|run(i)|**2)`` of the channel's samples, linear, in the units of the input samples -- read from the
        loaded spectrum without the inverse FFT.  Valid after ``load`` / ``adopt``; the channels may differ in bandwidth."""
        handle = self._ready()
        _, first, count = self._launch_plan()
        power = hip.empty((count,), self._torch.float32)
        hip.check(self._lib.rcfm_tuner_levels(handle, first, count, hip.ptr(power), hip.stream()))
        return self._out(power, numpy_output)

    # ---- carrier estimates and live retune (rcfm_tuner_carriers / rcfm_tuner_retune; no reference counterpart) --------

    def carriers(self, gate: float = 0.0, numpy_output: bool = True):
        """Where inside its channel each station sits: ``(peak_bin, peak_power, centroid, spread)``, one array of
        [count] each for every channel (of the shard's range after ``shard``), read from the loaded spectrum without the
        inverse FFT.  Offsets are bins from the channel centre -- Hz with one-second buffers: ``peak_bin`` (int32) the
        strongest bin, ``peak_power`` its power in the units of ``levels()`` per bin, ``centroid`` and ``spread`` the
        power-weighted mean and standard deviation over the bins whose power is at least ``gate`` (same units; 0 takes
        every bin, and a weak station's centroid is then pulled to 0 by the noise).  Valid after ``load`` / ``adopt``."""
        handle = self._ready()
        _, first, count = self._launch_plan()
        t = self._torch
        out = [hip.empty((count,), dt) for dt in (t.int32, t.float32, t.float32, t.float32)]
        hip.check(self._lib.rcfm_tuner_carriers(handle, first, count, float(gate), *[hip.ptr(o) for o in out], hip.stream()))
        return tuple(self._out(o, numpy_output) for o in out)

    def retune(self, offsets):
        """Move channel c up by ``offsets[c]`` bins (Hz with one-second buffers; a scalar moves every channel), on top of
        earlier retunes: a carrier that ``carriers()`` reported at ``peak_bin = k`` reads 0 after ``retune(k)``.  The
        device handle keeps its spectrum, plans and storage; after a plain ``load`` the same buffer can be run again at
        once, after a sharded load or ``adopt`` the next ``load`` / ``adopt`` must come first (RuntimeError until then),
        and while a window is attached the call is refused.  ``Channel`` objects and the input geometry do not change;
        ``add_channel`` and ``reset`` clear the fine-tune, ``fine_tune()`` returns it."""
        a = np.asarray(offsets)
        if a.dtype.kind not in "iu":
            if a.dtype.kind != "f" or not np.all(a == np.round(a)):
                raise ValueError("retune offsets are whole numbers of bins")
        a = self._per_channel(a, "retune offsets: a scalar or one per channel")
        fine = self.fine_tune() + np.broadcast_to(a, (len(self._bounds),)).astype(np.int64)    # (a new object per retune)
        if self._handle is not None and self._handle_key[1] == self._version:
            self._retune(self._handle.value, fine)               # (refused: the fine-tune in force stays)
            self._built["fine"] = (fine, self._handle_key, None)
        self._fine = fine

    def fine_tune(self):
        """int64 [len(channels())]: the bins every channel has been moved up by ``retune`` since the channel list last changed."""
        return np.zeros(len(self._bounds), np.int64) if self._fine is None else self._fine.copy()

    # ---- subcarrier tap (rcfm_pipeline_subcarrier; no reference counterpart) ---------------------------------------------

    def subcarrier(self, tap, first: int = 0, count: int = None, numpy_output: bool = True):
        """What else the FM multiplex of every channel carries: complex64 [count, tap.output_size], the baseband around the
        subcarrier of ``tap`` (a ``radiocore.analog.Subcarrier``: frequency, low-pass, output rate) for channels
        [first, first + count) of the loaded buffer (count None: up to the last channel), which must all have the tap's
        input size as bandwidth.  Valid after ``load`` / ``adopt``, on the current stream; it runs the channels' inverse
        FFT once more and touches no demodulator state, so it may come before or after ``run_all``.  RDS:
        ``radiocore.tools.rds`` decodes the 57 kHz tap on the host."""
        handle = self._ready()
        first = int(first)
        if count is None:                   # the rest of the tuner's channels, or of the shard's after ``shard``
            _, lo, n = self._launch_plan()
            first = max(first, lo)
            count = max(lo + n - first, 0)
        count = int(count)
        if first < 0 or count < 0 or first + count > len(self._bounds):
            raise IndexError("list index out of range")
        # one batched handle per (B, R, f, taps), sized for all channels like _batched_demod's: a longer channel list gets
        # a new one, the old one goes
        key = tap._key()
        held = self._taps.get(key)
        if held is None or held[0] < len(self._bounds):
            self._taps[key] = held = (len(self._bounds), tap._create(len(self._bounds), 0))
        out = hip.empty((count, tap._output_size), self._torch.complex64)
        hip.check(self._lib.rcfm_pipeline_subcarrier(handle, held[1].value, first, count, hip.ptr(out), hip.stream()))
        return self._out(out, numpy_output)

    def power_spectrum(self, cells, f_lo=None, f_hi=None, peak=False, numpy_output: bool = True):
        """What the band looks like between and around the channels (rcfm_tuner_power_spectrum; no reference
        counterpart): the loaded spectrum from ``f_lo`` to ``f_hi`` Hz (half-open; None: the band's own end) cut into
        ``cells`` cells of equal width to within one bin (``spectrum.cell_edges``), float32 [cells] -- the power in each
        cell, linear, in the units of the input samples and of ``levels()``; over the whole band the cells add up to
        ``mean(|x|**2)``.  peak=True returns ``(power, peak)``, peak being each cell's strongest bin: a narrow carrier
        stays visible in a wide cell.  Valid after ``load`` / ``adopt``; under ``shard`` or an attached window only
        the bins of ``window()`` are held and a span beyond them raises RuntimeError.  ValueError for an empty or
        out-of-band span and for ``cells`` outside 1 .. the span's bins."""
        if self._loaded_size is None:
            raise RuntimeError("Tuner.power_spectrum called before Tuner.load")
        s0, L = spectrum.span_bins(self._input_frequency, self._loaded_size, f_lo, f_hi)
        cells = int(cells)
        if cells < 1 or cells > L:
            raise ValueError("a span of %d bins takes 1 .. %d cells, not %d" % (L, L, cells))
        handle = self._ready()
        out = [hip.empty((cells,), self._torch.float32) for _ in range(2 if peak else 1)]
        hip.check(self._lib.rcfm_tuner_power_spectrum(handle, s0, L, cells, hip.ptr(out[0]), hip.ptr(out[1]) if peak else None,
                                                      hip.stream()))
        out = [self._out(o, numpy_output) for o in out]
        return (out[0], out[1]) if peak else out[0]

    # ---- IQ balance (rcfm_tuner_iq_estimate / _iq_correct / _set_iq_balance; no reference counterpart) -----------------

    def iq_imbalance(self, f_lo=None, f_hi=None, numpy_output: bool = True):
        """How far the receiver's I and Q paths are apart, read from the loaded buffer: ``(beta, sums)``.  A mismatch in
        gain and phase puts an image of every station at the mirrored frequency; ``beta`` (complex) is what
        ``set_iq_balance(beta)`` removes it with, ``sums`` (float64 [3]: Re P, Im P, Q) is what ``iq.balance_from``
        combines over several buffers.  ``f_lo`` / ``f_hi``: Hz above the input frequency, half-open like the span of
        ``power_spectrum`` -- the estimate uses the bins in that range together with their mirror images (None: from the
        first bin above the input frequency / up to the band's end).  The estimate is blind: two unmodulated carriers at
        exactly mirrored frequencies look like imbalance, so restrict it to a range the host trusts.  Valid after a plain
        ``load``; RuntimeError under ``shard``, after ``adopt`` or with a window attached (the mirror bins are elsewhere).
        On a ``cuda=True`` tuner ``numpy_output=False`` returns the device tensors (float32 [2], float64 [3]) unsynchronised."""
        if self._loaded_size is None:
            raise RuntimeError("Tuner.iq_imbalance called before Tuner.load")
        m_lo, m_hi = iq.pair_range(self._loaded_size, f_lo, f_hi)
        handle = self._ready()
        beta = hip.empty((2,), self._torch.float32)
        sums = hip.empty((3,), self._torch.float64)
        hip.check(self._lib.rcfm_tuner_iq_estimate(handle, m_lo, m_hi, hip.ptr(sums), hip.ptr(beta), hip.stream()))
        if self._cuda and not numpy_output:
            return beta, sums
        b = hip.to_host(beta)
        return complex(float(b[0]), float(b[1])), hip.to_host(sums)

    def set_iq_balance(self, balance=None, dc_notch: int = 0):
        """Image rejection on every buffer from now on: ``load`` / ``load_raw`` (and ``Lanes.submit``) queue the
        correction ``X[k] -= beta conj(X[-k])`` of the spectrum behind their FFT, on the device and on the caller's stream,
        and ``run`` / ``run_all`` / ``levels`` / squelch / ``power_spectrum`` / ``carriers`` / ``subcarrier`` see the clean
        band.  ``balance``: ``"auto"`` estimates beta blindly from each buffer itself; a complex number is a fixed beta
        (from ``iq_imbalance`` or ``iq.balance_from``: calibrate occasionally); ``None`` (the default) turns it off: nothing
        more is launched than before.  ``dc_notch = w`` zeroes the 2 w - 1 bins around the input frequency, where the
        receiver's DC offset sits (0: none).  ValueError for another string, a beta that is not finite or not below 1 in
        magnitude, a negative notch or one beyond half the band.  Needs the whole spectrum: ``load`` raises RuntimeError
        on a sharded tuner."""
        dc_notch = int(dc_notch)
        if dc_notch < 0:
            raise ValueError("dc_notch must be >= 0")
        if self._input_bandwidth and dc_notch > int(self._input_bandwidth) // 2:
            raise ValueError("dc_notch reaches beyond half the band")
        if balance is None:
            setting = None
        elif isinstance(balance, str):
            if balance != "auto":
                raise ValueError('set_iq_balance: None, "auto" or a complex beta, not %r' % (balance,))
            setting = (hip.RCFM_IQ_BALANCE_AUTO, 0j, dc_notch)
        else:
            try:
                beta = complex(balance)
            except (TypeError, ValueError):
                raise ValueError('set_iq_balance: None, "auto" or a complex beta, not %r' % (balance,))
            beta = complex(np.float32(beta.real), np.float32(beta.imag))     # what the device slot will hold
            if not (np.isfinite(beta.real) and np.isfinite(beta.imag)) or abs(beta) >= 1.0:
                raise ValueError("a fixed beta must be finite and below 1 in magnitude")
            setting = (hip.RCFM_IQ_BALANCE_FIXED, beta, dc_notch)
        self._iq_balance = setting
        if self._handle is not None and self._handle_key[1] == self._version:
            self._apply_iq_balance(self._handle.value)
            self._built["iq"] = (setting, self._handle_key, None)

    def _apply_iq_balance(self, handle):
        mode, beta, notch = self._iq_balance if self._iq_balance is not None else (hip.RCFM_IQ_BALANCE_OFF, 0j, 0)
        hip.check(self._lib.rcfm_tuner_set_iq_balance(handle, mode, beta.real, beta.imag, notch))

    # ---- noise blanker (rcfm_blanker_run ahead of the load; no reference counterpart) -----------------------------------

    def set_blanker(self, blanker=None, in_place=False):
        """Impulse noise taken out of every buffer from now on: with a ``radiocore.NoiseBlanker``, ``load`` / ``load_raw``
        (and ``Lanes.submit``) queue the blanker ahead of the wideband FFT -- and so ahead of the IQ balance, whose estimate
        sees the cleaned buffer -- on the caller's stream and without a host synchronisation; ``blanker_stats()`` tells what
        it did.  A host array is uploaded into a device tensor of its own anyway and is blanked in place there.  A caller's
        device tensor is left untouched: the tuner blanks it into a scratch tensor of the buffer's format and size, allocated
        by the first such load and kept (8 bytes per sample for complex64: 1.92 GB for a buffer of 2.4e8 samples) -- unless
        ``in_place=True``, which blanks the caller's tensor itself and needs no scratch.  ``shard``, ``whole=True``, attached
        spectra and windows are unaffected: the blanker acts on the input buffer, which every load has whole.  ``None``
        (the default) turns it off: nothing more is launched than before.  Each device tuner (each lane) keeps a blanker
        handle, and so the scratch of a run, of its own.  ValueError for anything but a NoiseBlanker, or one whose hold and
        ramp exceed 1024 samples of this tuner's buffers."""
        if blanker is None:
            self._blanker = None
            self._blank_handles = {}
            self._blank_scratch = None
            return
        if not hasattr(blanker, "geometry") or not hasattr(blanker, "_create"):
            raise ValueError("set_blanker takes a radiocore.NoiseBlanker")
        if self._input_bandwidth:
            blanker.geometry(int(self._input_bandwidth))
        self._blanker = (blanker, bool(in_place))

    def blanker_stats(self):
        """``(hits, blanked)`` of this tuner's last ``load`` / ``load_raw`` with a blanker set: the number of samples over
        the threshold and the number whose gain was below 1.  Waits for the device."""
        if self._blank_counts is None:
            raise RuntimeError("blanker_stats: no load with a blanker set (set_blanker) yet")
        c = hip.to_host(self._blank_counts)
        return int(c[0]), int(c[1])

    def _blank(self, x, n, fmt, upload):
        # ahead of the load on the same stream: x itself where it is this load's own upload (or in_place), else the scratch
        blanker, in_place = self._blanker
        blanker.geometry(n)
        ent = self._blank_handles.get(n)
        if ent is None or ent[0] is not blanker:
            ent = self._blank_handles[n] = (blanker, blanker._create(n))
        dst = x
        if not (upload or in_place):
            s = self._blank_scratch
            if s is None or s.dtype != x.dtype or tuple(s.shape) != tuple(x.shape):
                s = self._blank_scratch = hip.empty(tuple(x.shape), x.dtype)
            dst = s
        if self._blank_counts is None:
            self._blank_counts = hip.empty((2,), self._torch.int64)
        hip.check(self._lib.rcfm_blanker_run(ent[1].value, fmt, n, hip.ptr(x), hip.ptr(dst), hip.ptr(self._blank_counts),
                                             hip.stream()))
        return dst

    # ---- noise floor (rcfm_floor_run / rcfm_floor_thresholds behind the load; no reference counterpart) ------------------

    def set_floor(self, nf=None):
        """A noise floor that follows the band: with a ``radiocore.NoiseFloor``, every ``load`` / ``load_raw`` (and
        ``Lanes.submit``) queues three calls behind the wideband FFT and the IQ balance, on the caller's stream and without
        a host synchronisation: the power spectrum of the whole band in the floor's cells, the floor's order statistic and
        smoothing (its state is one per cell and buffer length, carried from buffer to buffer), and the thresholds of
        every channel -- the floor of the cell that holds the channel's centre, scaled to what ``levels()`` reads of white
        noise of that density in the channel's bandwidth.  ``set_squelch(OverFloor(db))`` and ``set_gate(gate,
        open=OverFloor(db))`` then compare against them; ``floor()``, ``floor_levels()`` and ``occupied_cells(db)`` read
        the last load's.  The state is zeroed ("not primed": the next buffer's estimate is taken as it is) by
        ``reset_states()`` and dropped by ``reset()`` and by another NoiseFloor.  ``None`` (the default) turns it off:
        nothing more is launched than before.  Needs the whole spectrum: ValueError here, or RuntimeError in ``load``, on a
        sharded tuner or with a spectrum or window attached.  ValueError for ``None`` while an ``OverFloor`` is in force, or
        a floor with fewer than guard + 2 cells in this tuner's band; the setting in force stays."""
        if nf is None:
            if isinstance(self._squelch, OverFloor) or (self._gate is not None and isinstance(self._gate[1], OverFloor)):
                raise ValueError("set_floor(None): an OverFloor threshold is in force (set_squelch / set_gate); turn it off first")
        else:
            if not hasattr(nf, "cells") or not hasattr(nf, "_create"):
                raise ValueError("set_floor takes a radiocore.NoiseFloor")
            try:
                self._floor_whole("set_floor")
            except RuntimeError as e:
                raise ValueError(str(e))
            if self._input_bandwidth and nf.cells(int(self._input_bandwidth)) < nf.guard + 2:
                raise ValueError("set_floor: %d cells are fewer than guard + 2" % nf.cells(int(self._input_bandwidth)))
        if nf is not self._floor:
            self._floor_handles.clear()            # another floor: no cell is primed
            self._floor_out = None
        self._floor = nf

    def _floor_whole(self, what):
        if self._shard is not None or getattr(self, "_slot", None) is not None:
            raise RuntimeError("%s: the noise floor needs the whole spectrum, not a shard's or an attached one" % what)

    def _floor_dbs(self):
        # the dB figures the load makes thresholds for: 0 (floor_levels) and whatever squelch and gate ask for
        dbs = [0.0]
        for a in (self._squelch,) + (tuple(self._gate[1:]) if self._gate is not None else ()):
            if isinstance(a, OverFloor) and a.db not in dbs:
                dbs.append(a.db)
        return tuple(dbs)

    def _floor_tables(self, n, dbs):
        """(cell int32 [K C], gain float32 [K C]) on the device for the K figures of dbs, figure after figure: cell[c] is
        the cell that holds the channel's centre bin (-1 when that lies outside the band: a NaN threshold, the channel stays
        closed), gain[c] = G(B_c) / len(cell) 10^(db / 10) in float64, rounded once."""
        def make():
            C, M = len(self._bounds), self._floor.cells(n)
            edges = spectrum.cell_edges(n, M)
            centre = -np.array(list(self._rolls(self._fine)), dtype=np.int64) + n // 2      # span position of every centre bin
            inside = (centre >= 0) & (centre < n)
            cell = np.where(inside, np.searchsorted(edges, centre, side="right") - 1, -1).astype(np.int32)
            width = np.diff(edges)[np.clip(cell, 0, M - 1)].astype(np.float64)
            gains = {}
            G = np.array([gains.setdefault(B, channel_noise_gain(B, n)) for B in (int(ch.bandwidth) for ch in self._bounds)])
            gain = np.concatenate([(G / width * 10.0 ** (db / 10.0)).astype(np.float32) for db in dbs]) if C else np.zeros(0, np.float32)
            return hip.to_device(np.tile(cell, len(dbs)), self._torch.int32), hip.to_device(gain, self._torch.float32)
        fine = None if self._fine is None else self._fine.tobytes()
        return self._derived("floor tables %r" % (dbs,), self._floor, (self._version, n, fine), make)

    def _floor_handle(self, n):
        # one handle per buffer length, shared with the lanes: the tracked floor is the band's, whoever loads the buffer
        nf = self._floor
        ent = self._floor_handles.get(n)
        if ent is None or ent[0] is not nf:
            ent = self._floor_handles.put(n, (nf, nf._create(nf.cells(n))), self._state_fence)
        return ent[1].value

    def _floor_pass(self, handle, n):
        # behind the load (FFT and IQ balance) on the same stream: power spectrum, floor, thresholds
        M = self._floor.cells(n)
        t, s = self._torch, hip.stream()
        power, floor = hip.empty((M,), t.float32), hip.empty((M,), t.float32)
        hip.check(self._lib.rcfm_tuner_power_spectrum(handle, -(n // 2), n, M, hip.ptr(power), None, s))
        hip.check(self._lib.rcfm_floor_run(self._floor_handle(n), hip.ptr(power), 1.0, hip.ptr(floor), None, s))
        self._floor_out = (n, M, power, floor, {})
        self._floor_queue(self._floor_dbs())

    def _floor_queue(self, dbs):
        # rcfm_floor_thresholds of the last load's floor for every figure of dbs, one call
        n, M, _, floor, held = self._floor_out
        C = len(self._bounds)
        cell, gain = self._floor_tables(n, dbs)
        thr = hip.empty((len(dbs) * C,), self._torch.float32)
        hip.check(self._lib.rcfm_floor_thresholds(hip.ptr(floor), M, hip.ptr(cell), hip.ptr(gain), len(dbs) * C, hip.ptr(thr),
                                                  hip.stream()))
        for k, db in enumerate(dbs):
            held[db] = _Part(thr, k * C, C)

    def _floor_thresholds(self, db):
        """The last load's thresholds ``db`` over the floor, float32 [len(channels())] on the device (a _Part): made by the
        load for the figures in force then, and from its floor now for one that was set since."""
        if self._floor is None or self._floor_out is None or self._floor_out[0] != self._loaded_size:
            raise RuntimeError("an OverFloor threshold needs a load with the noise floor set (set_floor)")
        held = self._floor_out[4]
        if db not in held:
            self._floor_queue((db,))
        return held[db]

    def _floor_read(self, what):
        if self._floor_out is None:
            raise RuntimeError("%s: no load with a noise floor set (set_floor) yet" % what)
        return self._floor_out

    def floor(self, numpy_output: bool = True):
        """float32 [cells]: the tracked noise floor of every cell after this tuner's last ``load`` with a floor set, in the
        units of ``power_spectrum(cells)`` -- power per cell."""
        return self._out(self._floor_read("floor")[3], numpy_output)

    def floor_levels(self, numpy_output: bool = True):
        """float32 [len(channels())]: what ``levels()`` would read of every channel if it held nothing but the noise floor
        of its cell -- ``OverFloor(0)``."""
        self._floor_read("floor_levels")
        return self._out(self._floor_thresholds(0.0).tensor(), numpy_output)

    def occupied_cells(self, db):
        """numpy bool [cells]: the cells of the last load whose power is at least ``db`` dB over their tracked floor -- the
        rule of rcfm_floor_run's ``over``, ``power >= float32(10 ** (db / 10)) * floor`` in float32, false on NaN."""
        _, _, power, floor, _ = self._floor_read("occupied_cells")
        ratio = np.float32(10.0 ** (float(db) / 10.0))
        with np.errstate(invalid="ignore"):
            return hip.to_host(power) >= ratio * hip.to_host(floor)

    def set_squelch(self, threshold=None):
        """Mute what is below a level: from now on ``run_all`` / ``run_each`` (and ``Lanes.submit``) compare every
        channel's level of the buffer with its threshold -- a scalar, or a sequence of ``len(channels())``, in the units
        of ``levels()`` -- and return exact zeros for the channels below it; ``open_mask()`` tells which were open.  The
        decision is per buffer, on the device and on the caller's stream (no host synchronisation), and the
        demodulators still run on every channel: the de-emphasis state advances as without squelch.  A NaN threshold
        keeps a channel closed.  ``None`` (the default) turns squelch off: nothing more is launched than before.
        ``squelch.threshold_over_floor`` derives thresholds from a ``levels()`` pass; with a noise floor set (``set_floor``)
        ``OverFloor(db)`` stands for "db over the floor at each channel, as the buffer's load tracked it" and needs no such
        pass.  ValueError while a frame gate is set (``set_gate``): the two take the same place; and for an ``OverFloor``
        without ``set_floor``; the setting in force stays."""
        if threshold is not None and self._gate is not None:
            raise ValueError("set_squelch: a frame gate is set (set_gate); turn it off first")
        if isinstance(threshold, OverFloor):
            if self._floor is None:
                raise ValueError("set_squelch: OverFloor needs a noise floor (set_floor)")
            self._squelch = OverFloor(threshold.db)                                # (a new object per setting)
        else:
            self._squelch = None if threshold is None else self._per_channel(    # (np.array: a copy, a new object per setting)
                np.array(threshold, dtype=np.float32), "squelch thresholds: a scalar or one per channel")
        self._last = self._last._replace(masks=None)

    def open_mask(self):
        """numpy bool [count]: which channels the squelch -- the level squelch, the tone squelch, or both combined -- left
        open in this tuner's last ``run_all`` / ``run_each``."""
        if self._last.masks is None:
            raise RuntimeError("open_mask: no run_all / run_each with squelch set (set_squelch) yet")
        return self._mask_result(self._last.masks)

    @staticmethod
    def _mask_result(masks):
        return np.concatenate([hip.to_host(m) for m in masks]).astype(bool) if masks else np.zeros(0, bool)

    # ---- tone bank and tone squelch (rcfm_tone_bank_run / rcfm_tone_score; no reference counterpart) ---------------------

    def set_tones(self, bank=None, want=None, ratio=None):
        """Signalling tones on the audio: with a ``radiocore.ToneBank``, ``run_all`` / ``run_each`` / ``run_all_packed`` (and
        ``Lanes.submit``) queue the bank behind the demodulators of each group, on the caller's stream and without a host
        synchronisation, and ``tone_power()`` returns what it measured: per channel and frame the power at each of the
        bank's tones and the frame's total power.  It runs before the level squelch, on the left side of WBFM's stereo.
        With ``want`` and ``ratio`` it is a tone squelch as well: a channel stays open only when, in some frame, the share
        ``P / E`` of its wanted tone reaches its ratio -- and when the level squelch, if one is set, leaves it open;
        everything else comes back as exact zeros and ``open_mask()`` returns the combined mask.  ``want``: one entry per
        channel or one for all, a tone index (int), a frequency of the bank in Hz (float), or None / -1 for "no tone
        needed"; ``ratio``: a scalar or one per channel.  ``None`` (the default) turns it all off: nothing more is launched
        than before.  ValueError, here or -- for channels added later -- in the next run before anything of it is launched,
        for a bank that does not fit a channel's audio: a frame longer than the audio, a tone above half its rate, a window
        of another length or without a positive sum; the setting in force stays."""
        C = len(self._bounds)
        if bank is None:
            if want is not None or ratio is not None:
                raise ValueError("set_tones: want and ratio need a bank")
            self._tones = None
        else:
            if (want is None) != (ratio is None):
                raise ValueError("set_tones: a tone squelch takes both want and ratio")
            w = r = None
            if ratio is not None:
                if isinstance(want, (list, tuple, np.ndarray)):
                    if len(want) != C:
                        raise ValueError("wanted tones: one for all or one per channel (%d)" % C)
                    w = np.array([bank.index(v.item() if isinstance(v, np.generic) else v) for v in want], dtype=np.int32)
                else:
                    w = np.full(C, bank.index(want), dtype=np.int32)
                r = self._per_channel(np.array(ratio, dtype=np.float32), "tone ratios: a scalar or one per channel")
                r = np.array(np.broadcast_to(r, (C,)))           # (a copy: writable, contiguous)
            setting = (bank, w, r)
            self._fit_tones(setting)               # refused here, with the old setting still in force
            self._tones = setting
        self._last = _Run()

    def _fit(self, name, setting, check):
        """``check(the audio lengths of the launch plan's groups, ascending)`` once per (channel list, shard, setting): what
        does not fit these channels raises there, before a run has advanced any state."""
        if setting is not None and self._bounds:
            groups, _, _ = self._launch_plan()
            self._derived(name, setting, self._plan[0], lambda: check(sorted({g[4] for g in groups if g[2] is not None})))

    def _fit_tones(self, setting):
        """The bank's device handle for the audio length of every group of the launch plan, made now: whatever is wrong
        with the bank for these channels raises here, before a run has advanced any demodulator state."""
        self._fit("tones fit", setting, lambda lengths: [setting[0]._handle(A) for A in lengths])

    def tone_power(self, numpy_output: bool = True):
        """``(P [count, F, K], E [count, F])`` of this tuner's last ``run_all`` / ``run_each`` with a tone bank set: the
        power at each tone and the total power of every frame of every channel.  (``run_each`` over groups whose audio
        lengths give different frame counts: a list with one such pair per group.)"""
        if self._last.tones is None:
            raise RuntimeError("tone_power: no run_all / run_each with a tone bank set (set_tones) yet")
        return self._tone_result(self._last.tones, self._cuda and not numpy_output)

    def _tone_result(self, pairs, device_output):
        t = self._torch
        if len({tuple(p.shape[1:]) for p, _ in pairs}) > 1:
            return [(self._result(p, device_output), self._result(e, device_output)) for p, e in pairs]
        P = pairs[0][0] if len(pairs) == 1 else t.cat([p for p, _ in pairs])
        E = pairs[0][1] if len(pairs) == 1 else t.cat([e for _, e in pairs])
        return self._result(P, device_output), self._result(E, device_output)

    def _tone_squelch(self, first, count, audio, tones, gate):
        # behind the group's tone bank (and level squelch): the wanted tone's best share, then mask + zero fill on it
        bank, want, ratio = self._tones

        def upload():
            if want.shape[0] != len(self._bounds):
                raise ValueError("wanted tones were set for %d channels, the tuner has %d" % (want.shape[0], len(self._bounds)))
            return hip.to_device(want, self._torch.int32), hip.to_device(ratio, self._torch.float32)
        want_dev, ratio_dev = self._derived("tone squelch", self._tones, self._version, upload)
        P, E = tones
        score = hip.empty((count,), self._torch.float32)
        mask = hip.empty((count,), self._torch.uint8)
        s = hip.stream()
        hip.check(self._lib.rcfm_tone_score(hip.ptr(P), hip.ptr(E), ctypes.c_void_p(want_dev.data_ptr() + 4 * first),
                                            hip.ptr(gate) if gate is not None else None, count, int(P.shape[1]),
                                            int(P.shape[2]), hip.ptr(score), s))
        hip.check(self._lib.rcfm_squelch(hip.ptr(score), ctypes.c_void_p(ratio_dev.data_ptr() + 4 * first), count,
                                         audio.numel() // count, hip.ptr(audio), hip.ptr(mask), s))
        return mask

    # ---- audio filter (rcfm_audio_filter_run; no reference counterpart) ------------------------------------------------

    def set_audio_filter(self, filt=None, channels=None):
        """What a receiver applies to the audio before its speaker: with a ``radiocore.AudioFilter`` (for instance
        ``radiocore.tools.audiofilter.VOICE_NFM``: the 300 Hz high-pass that strips the CTCSS tone, a 3 kHz low-pass and
        narrow FM's de-emphasis), ``run_all`` / ``run_each`` / ``run_all_packed`` (and ``Lanes.submit``) filter every
        group's audio in place behind its demodulators, on the caller's stream and without a host synchronisation.  The
        filter runs behind the tone bank -- ``tone_power()`` sees the unfiltered audio -- and before the level squelch and
        the tone squelch zero the closed rows; its state is one per channel (and leg), carried from buffer to buffer
        whether the channel is open or not, kept when channels are added, zeroed by ``reset_states()`` and dropped by
        ``reset()`` and by a new filter.  ``channels``: a bool per channel, or None for all.  ``None`` (the default) turns
        it off: nothing more is launched than before.  ValueError, here or -- for channels added later -- in the next run
        before anything of it is launched, for a filter without a design at a channel's audio rate (a corner at or above
        half of it, ``sos`` sections of another rate) or a selection of another length; the setting in force stays."""
        if filt is None:
            if channels is not None:
                raise ValueError("set_audio_filter: channels need a filter")
            self._afilt = None
            self._afilt_handles.clear()
        else:
            if not hasattr(filt, "sections") or not hasattr(filt, "_create"):
                raise ValueError("set_audio_filter takes a radiocore.AudioFilter")
            sel = None
            if channels is not None:
                sel = self._per_channel(np.array(channels, dtype=bool).astype(np.uint8),
                                        "filtered channels: one bool per channel", scalar=False)
            setting = (filt, sel)
            self._fit_afilt(setting)               # refused here, with the old setting still in force
            if self._afilt is None or self._afilt[0] is not filt:
                self._afilt_handles.clear()        # another filter: its states start at rest
            self._afilt = setting

    def _fit_afilt(self, setting):
        """The filter's design for the audio rate of every group of the launch plan, and the selection's length: whatever
        is wrong raises here, before a run has advanced any state."""
        def check(lengths):
            if setting[1] is not None and setting[1].shape[0] != len(self._bounds):
                raise ValueError("filtered channels were set for %d channels, the tuner has %d" % (setting[1].shape[0], len(self._bounds)))
            for A in lengths:
                setting[0].sections(A)
        self._fit("filter fit", setting, check)

    def _channel_states(self, cache, key, owner, create, shape, ctype, get_state, set_state):
        """The handle cache[key] -> (channels, owner, handle) of a stage with one state of `shape` (of `ctype`) per channel:
        ``create(C)``, sized for all channels -- the state slots are addressed by channel index, so shard and regrouping keep
        them -- and made again for a longer channel list, which takes the states over, or, at rest, for another owner."""
        C = len(self._bounds)
        ent = cache.get(key)
        if ent is None or ent[0] != C or ent[1] is not owner:
            h = create(C)
            if ent is not None and ent[1] is owner:
                p = ctypes.POINTER(ctype)
                old = np.zeros((ent[0],) + shape, ctype)
                hip.check(get_state(ent[2].value, old.ctypes.data_as(p), hip.stream()))
                new = np.zeros((C,) + shape, ctype)
                new[:min(C, ent[0])] = old[:min(C, ent[0])]
                hip.check(set_state(h.value, new.ctypes.data_as(p), hip.stream()))
            ent = cache.put(key, (C, owner, h), self._state_fence)
        return ent[2].value

    def _afilt_handle(self, ch, A):
        filt = self._afilt[0]               # one handle per (legs, audio rate)
        return self._channel_states(self._afilt_handles, (ch, A), filt, lambda C: filt._create(C, ch, A), (ch, len(filt), 2),
                                    ctypes.c_double, self._lib.rcfm_audio_filter_get_state, self._lib.rcfm_audio_filter_set_state)

    def _filter_group(self, first, count, audio):
        # behind the group's tone bank on the same stream, in place
        sel = None
        if self._afilt[1] is not None:
            dev = self._derived("filter selection", self._afilt, self._version, lambda: hip.to_device(self._afilt[1]))
            sel = ctypes.c_void_p(dev.data_ptr() + first)
        A, ch = int(audio.shape[1]), int(audio.shape[2])
        hip.check(self._lib.rcfm_audio_filter_run(self._afilt_handle(ch, A), first, count, A, hip.ptr(audio), hip.ptr(audio),
                                                  sel, hip.stream()))

    # ---- frame levels and the frame gate (rcfm_tuner_frame_levels / rcfm_gate_*; no reference counterpart) ---------------

    def _bandwidth_runs(self):
        """[(first, count, B)]: the runs of consecutive channels of one bandwidth in the launch plan's range, once per
        (channel list, shard)."""
        def make():
            _, first, count = self._launch_plan()
            runs, i = [], first
            while i < first + count:
                B, j = int(self._bounds[i].bandwidth), i + 1
                while j < first + count and int(self._bounds[j].bandwidth) == B:
                    j += 1
                runs.append((i, j - i, B))
                i = j
            return runs
        self._launch_plan()
        return self._derived("bandwidth runs", None, self._plan[0], make)

    def _frame_levels(self, handle, first, count, B, F, power_ptr):
        # rcfm_tuner_frame_levels of one run of like channels on the current stream, through this device tuner's scratch
        m = max(1, min(count, _FRAME_SCRATCH_BYTES // (8 * B)))
        s = self._frame_scratch
        if s is None or int(s.numel()) < m * B:
            s = self._frame_scratch = hip.empty((m * B,), self._torch.complex64)
        hip.check(self._lib.rcfm_tuner_frame_levels(handle, first, count, F, hip.ptr(s), ctypes.c_size_t(8 * int(s.numel())),
                                                    power_ptr, hip.stream()))

    def frame_levels(self, frames, numpy_output: bool = True):
        """``levels()`` resolved in time: float32 [count, frames], the mean power of each of the ``frames`` equal frames of
        every channel's samples of the loaded buffer (of the shard's range after ``shard``), in the units of ``levels()``;
        the mean over a channel's frames is its level.  A read like ``levels()``: valid after ``load`` / ``adopt``, it needs
        no gate and touches no state.  It runs the channels' inverse FFT once more, a chunk of channels at a time through a
        scratch of at most 256 MB that the tuner keeps.  ValueError unless ``frames`` divides every channel's bandwidth."""
        handle = self._ready()
        F = int(frames)
        if F != frames or F < 1:
            raise ValueError("frames: a positive integer, not %r" % (frames,))
        _, first, count = self._launch_plan()
        runs = self._bandwidth_runs()
        for _, _, B in runs:
            if B % F:
                raise ValueError("%d frames do not divide a channel of %d samples" % (F, B))
        power = hip.empty((count, F), self._torch.float32)
        for lo, n, B in runs:
            self._frame_levels(handle, lo, n, B, F, ctypes.c_void_p(power.data_ptr() + 4 * F * (lo - first)))
        return self._out(power, numpy_output)

    def set_gate(self, gate=None, open=None, close=None, hysteresis_db: float = 3.0):
        """A squelch that is right to a frame, not to a buffer: with a ``radiocore.FrameGate``, ``run_all`` / ``run_each`` /
        ``run_all_packed`` (and ``Lanes.submit``) measure every frame of every channel (``frame_levels``), walk the gate's
        state machine over them -- open at ``open``, held at ``close``, hang time, look-ahead -- and zero the closed frames
        of the audio with a short fade at the edges, on the device and on the caller's stream, in the level squelch's place:
        behind the tone bank and the audio filter, ahead of the tone squelch.  ``open_mask()`` tells which channels had
        anything open in the buffer (``run_all_packed``, the ``Drain`` and ``wire.frames_packed`` work on it unchanged),
        ``frame_mask()`` which frames.  ``open`` and ``close``: in the units of ``levels()``, a scalar or one per channel
        (``squelch.threshold_over_floor`` gives ``open``), or -- with ``set_floor`` -- ``OverFloor(db)`` for both, the
        thresholds the buffer's load made from the tracked noise floor; ``close`` defaults to ``open`` lowered by ``hysteresis_db``.  The
        state is one per channel, carried from buffer to buffer, kept when channels are added, zeroed by ``reset_states()``
        and dropped by ``reset()`` and by another gate.  ``None`` (the default) turns it off: nothing more is launched than
        before.  ValueError -- the setting in force stays -- for ``close`` above ``open``, while ``set_squelch`` is set, and,
        here or for channels added later in the next run before anything of it is launched, for frames that do not
        divide a channel's bandwidth or audio length, or thresholds of another length."""
        if gate is None:
            if open is not None or close is not None:
                raise ValueError("set_gate: thresholds need a gate")
            self._gate = None
            self._gate_handles.clear()
        else:
            if not hasattr(gate, "ramp_array") or not hasattr(gate, "_create"):
                raise ValueError("set_gate takes a radiocore.FrameGate")
            if self._squelch is not None:
                raise ValueError("set_gate: a level squelch is set (set_squelch); turn it off first")
            if open is None:
                raise ValueError("set_gate: a gate needs its open threshold")
            what = "gate thresholds: a scalar or one per channel"
            if isinstance(open, OverFloor) or isinstance(close, OverFloor):
                if self._floor is None:
                    raise ValueError("set_gate: OverFloor needs a noise floor (set_floor)")
                if not isinstance(open, OverFloor) or not (close is None or isinstance(close, OverFloor)):
                    raise ValueError("set_gate: open and close are both levels or both OverFloor")
                o = OverFloor(open.db)
                c = OverFloor(open.db - float(hysteresis_db) if close is None else close.db)
                if c.db > o.db:
                    raise ValueError("set_gate: close lies above open")
            else:
                o = self._per_channel(np.array(open, dtype=np.float32), what)
                if close is None:
                    c = (o.astype(np.float64) * 10.0 ** (-float(hysteresis_db) / 10.0)).astype(np.float32)
                else:
                    c = self._per_channel(np.array(close, dtype=np.float32), what)
                if np.any(c > o):
                    raise ValueError("set_gate: close lies above open")
            setting = (gate, o, c)
            self._fit_gate(setting)                # refused here, with the old setting still in force
            if self._gate is None or self._gate[0] is not gate:
                self._gate_handles.clear()         # another gate: every channel starts closed
            self._gate = setting
        self._last = self._last._replace(masks=None, frames=None)

    def _fit_gate(self, setting):
        """The gate's frames against the bandwidth and audio length of every group of the launch plan, and the thresholds'
        length: whatever is wrong raises here, before a run has advanced any state."""
        if setting is None or not self._bounds:
            return

        def check():
            gate, C = setting[0], len(self._bounds)
            for a in setting[1:]:
                if not isinstance(a, OverFloor) and a.ndim == 1 and a.shape[0] != C:
                    raise ValueError("gate thresholds were set for %d channels, the tuner has %d" % (a.shape[0], C))
            for g in self._launch_plan()[0]:
                if g[2] is not None:
                    gate.fits(g[3])
                    gate.ramp_samples(g[4])
        self._launch_plan()
        self._derived("gate fit", setting, self._plan[0], check)

    def frame_mask(self):
        """numpy bool [count, frames]: which frames of which channels the frame gate left open in this tuner's last
        ``run_all`` / ``run_each`` -- look-ahead included, the tone squelch's verdict not (``open_mask()`` has that)."""
        if self._last.frames is None:
            raise RuntimeError("frame_mask: no run_all / run_each with a frame gate set (set_gate) yet")
        return self._frame_result(self._last.frames)

    @staticmethod
    def _frame_result(frames):
        return np.concatenate([hip.to_host(m)[:, 1:] for m in frames]).astype(bool)

    def _gate_handle(self, A):
        gate = self._gate[0]                # one handle per audio rate (the fade's length follows it)
        return self._channel_states(self._gate_handles, A, gate, lambda C: gate._create(C, A), (2,), ctypes.c_int32,
                                    self._lib.rcfm_gate_get_state, self._lib.rcfm_gate_set_state)

    def _gate_group(self, handle, first, count, audio):
        # behind the group's audio filter on the same stream: frame levels of its channels, the state machine, then the
        # zero fill and fades in place.  (open_any uint8 [count], frame mask uint8 [count, F + 1])
        def upload():
            C = len(self._bounds)
            return tuple(hip.to_device(np.array(np.broadcast_to(a, (C,))), self._torch.float32) for a in self._gate[1:])    # (a copy: writable)
        if isinstance(self._gate[1], OverFloor):
            thr_open, thr_close = self._floor_thresholds(self._gate[1].db), self._floor_thresholds(self._gate[2].db)
        else:
            thr_open, thr_close = self._derived("gate thresholds", self._gate, self._version, upload)
        F = self._gate[0].frames
        A, ch = int(audio.shape[1]), int(audio.shape[2])
        t = self._torch
        power = hip.empty((count, F), t.float32)
        fmask = hip.empty((count, F + 1), t.uint8)
        mask = hip.empty((count,), t.uint8)
        g, s = self._gate_handle(A), hip.stream()
        self._frame_levels(handle, first, count, int(self._bounds[first].bandwidth), F, hip.ptr(power))
        hip.check(self._lib.rcfm_gate_run(g, first, count, F, hip.ptr(power), ctypes.c_void_p(thr_open.data_ptr() + 4 * first),
                                          ctypes.c_void_p(thr_close.data_ptr() + 4 * first), hip.ptr(fmask), hip.ptr(mask), s))
        hip.check(self._lib.rcfm_gate_apply(g, hip.ptr(fmask), count, F, A, ch, hip.ptr(audio), s))
        return mask, fmask

    # ---- audio buses (rcfm_mix_run behind everything else of a group; no reference counterpart) -------------------------

    def set_mix(self, mixer=None):
        """The open channels mixed to a few streams: with a ``radiocore.Mixer``, ``run_all`` / ``run_each`` /
        ``run_all_packed`` (and ``Lanes.submit``) queue the mixer behind everything else of each group -- the tone bank, the
        audio filter, the level squelch or the frame gate, the tone squelch -- on their final open mask, on the caller's
        stream and without a host synchronisation: every bus is the sum of its open channels' audio at the routes' gains,
        in the one order the route list fixes (include/rcfm.h, "audio buses"); a closed channel is not read.  ``mix()``
        returns the buses of the last run, ``mix_active()`` how many channels each had open, and
        ``run_all_packed(pcm, drain=..., buses=True)`` packs and drains the bus rows instead of the channel rows.  The
        channel audio itself is what it is without a mixer.  ``run_each`` mixes per group of like channels: a bus takes
        channels of one group, and buses of different groups may differ in length.  Routes name channel indices, so a
        channel list that grows keeps working.  ``None`` (the default) turns it off: nothing more is launched than before.
        ValueError -- the setting in force stays -- for anything but a Mixer, for a route to a channel the tuner does not
        have (here, and in a run after ``reset()``, before anything is launched), for a bus across two groups (in
        ``run_each``, before anything is launched), on a sharded tuner or with a spectrum or window attached."""
        if mixer is not None:
            if not hasattr(mixer, "buses") or not hasattr(mixer, "_split"):
                raise ValueError("set_mix takes a radiocore.Mixer")
            try:
                self._mix_whole("set_mix")
            except RuntimeError as e:
                raise ValueError(str(e))
            if self._bounds and mixer.highest_channel() >= len(self._bounds):
                raise ValueError("set_mix: a route names channel %d, the tuner has %d channels"
                                 % (mixer.highest_channel(), len(self._bounds)))
            if self._busdyn is not None and self._busdyn[1] is not None:
                busdyn.resolve_ducks(self._busdyn[1], mixer.buses)     # the ducks in force must name buses of the new mixer
        if mixer is not self._mix:
            self._mix_handles.clear()              # another mixer: other tables
            self._busdyn_handles.clear()           # ... and other buses: their dynamics start at rest
        if mixer is None:
            self._busdyn = None                    # the dynamics go with the buses (set_bus_dynamics needs a mixer)
        self._mix = mixer
        self._last = self._last._replace(mix=None, dry=None)

    def _mix_whole(self, what):
        if self._shard is not None or getattr(self, "_slot", None) is not None:
            raise RuntimeError("%s: the mixer takes every channel of the tuner, not a shard's or an attached window's" % what)

    def _fit_mix(self, ranges):
        """(owner [M], [librcfm handle per group]) of the mixer for the launch groups ``ranges`` ((first, count), ..): made
        once per mixer, channel-list version and grouping, before a run has launched anything -- whatever is wrong with the
        routes for these channels raises here."""
        self._mix_whole("run")
        mixer = self._mix
        ent = self._mix_handles.get(ranges)
        if ent is None or ent[0] is not mixer or ent[1] != self._version:
            owner, tables = mixer._split(ranges, len(self._bounds))
            for key in [k for k, e in self._mix_handles.items() if e[1] != self._version]:
                del self._mix_handles[key]         # the handles of a channel list that is gone
            ent = self._mix_handles.put(ranges, (mixer, self._version, owner, [mixer._create(*t) for t in tables]), self._state_fence)
        return ent[2], [h.value for h in ent[3]]

    def _mix_group(self, h, first, count, audio, mask):
        # behind the group's squelch / gate / tone squelch on the same stream, on their final mask (None: every channel open)
        M, ch_out = self._mix.M, self._mix.ch_out
        A, ch = int(audio.shape[1]), int(audio.shape[2])
        t = self._torch
        out = hip.empty((M, A, ch_out), t.float32)
        active = hip.empty((M,), t.int32)
        bus_open = hip.empty((M,), t.uint8)
        hip.check(self._lib.rcfm_mix_run(h, first, count, A, ch, hip.ptr(audio), hip.ptr(mask) if mask is not None else None,
                                         hip.ptr(out), hip.ptr(active), hip.ptr(bus_open), hip.stream()))
        return out, active, bus_open

    def mix(self, numpy_output: bool = True, dry: bool = False):
        """The buses of this tuner's last ``run_all`` / ``run_each`` / ``run_all_packed`` with a mixer set, float32
        [M, A, ch_out].  After a ``run_each`` over several groups: a list with one [A, ch_out] array per bus (the groups'
        audio lengths may differ; a bus without a route has the first group's).  With ``set_bus_dynamics`` these are the
        processed rows, ``bus_delay()`` samples late; ``dry=True`` returns the mixer's own rows."""
        if self._last.mix is None:
            raise RuntimeError("mix: no run_all / run_each with a mixer set (set_mix) yet")
        which = self._last.dry if dry and self._last.dry is not None else self._last.mix
        return self._mix_result(which, self._cuda and not numpy_output)

    def _mix_result(self, mix, device_output):
        owner, groups = mix
        if len(groups) == 1:
            return self._result(groups[0][0], device_output)
        outs = [self._result(g[0], device_output) for g in groups]
        return [outs[k][m] for m, k in enumerate(owner)]

    def mix_active(self):
        """numpy int32 [M]: how many routes of each bus were open in this tuner's last run with a mixer set."""
        if self._last.mix is None:
            raise RuntimeError("mix_active: no run_all / run_each with a mixer set (set_mix) yet")
        return self._mix_active_result(self._last.mix)

    @staticmethod
    def _mix_active_result(mix):
        owner, groups = mix
        active = [np.asarray(hip.to_host(g[1])) for g in groups]
        return np.array([active[k][m] for m, k in enumerate(owner)], dtype=np.int32)

    # ---- bus dynamics (rcfm_busdyn_run behind rcfm_mix_run of a group; no reference counterpart) ------------------------

    def set_bus_dynamics(self, limiter=None, ducks=None):
        """A look-ahead peak limiter, and ducking, on the buses of ``set_mix``: with a ``radiocore.Limiter``, ``run_all`` /
        ``run_each`` / ``run_all_packed`` (and ``Lanes.submit``) queue rcfm_busdyn_run right behind the mixer of each group,
        on the caller's stream and without a host synchronisation (include/rcfm.h, "bus dynamics").  No sample of ``mix()``
        then exceeds the limiter's ceiling, every bus comes ``bus_delay()`` samples late, and ``mix(dry=True)`` still returns
        the mixer's own rows; ``run_all_packed(buses=True)`` packs the processed rows, and a bus that has gone idle stays
        open for one more buffer while its tail drains.  ``ducks``: ``{bus index or name: radiocore.Duck}`` -- that bus is
        turned down while the duck's key bus is active; the key must lie in the same launch group of ``run_each``.  The state
        (tail, gain, hang) is one per bus, carried from buffer to buffer, kept while the groups' audio lengths stay the same,
        zeroed by ``reset_states()`` and dropped by ``reset()``, by another mixer and by new settings here.  Limiter and
        ducks are discretised at each group's audio rate.  No arguments: off, nothing more is launched than before.
        ValueError -- the setting in force stays -- without a mixer, for ducks without a limiter, for anything but a Limiter
        and Ducks, for a bus or key the mixer does not have, on a sharded tuner or with a spectrum or window attached."""
        if limiter is None:
            if ducks:
                raise ValueError("set_bus_dynamics: ducks need a limiter (its look-ahead and release shape them)")
            setting = None
        else:
            if not isinstance(limiter, busdyn.Limiter):
                raise ValueError("set_bus_dynamics takes a radiocore.Limiter")
            if self._mix is None:
                raise ValueError("set_bus_dynamics needs a mixer first (set_mix)")
            try:
                self._mix_whole("set_bus_dynamics")
            except RuntimeError as e:
                raise ValueError(str(e))
            ducks = dict(ducks) if ducks else None
            if ducks is not None:
                busdyn.resolve_ducks(ducks, self._mix.buses)
            setting = (limiter, ducks)
        self._busdyn_handles.clear()               # new settings: the dynamics start at rest
        self._busdyn = setting
        self._last = self._last._replace(dry=None)

    def _fit_busdyn(self, owner, groups):
        """[(L, librcfm handle)] per launch group for the bus dynamics in force, made before a run has launched anything:
        a duck across two groups raises here.  One handle per group, every bus in each (a bus of another group is a row of
        +0 there); kept while the mixer's shape and the groups' audio lengths stay what they are."""
        limiter, ducks = self._busdyn
        M, ch_out = self._mix.M, self._mix.ch_out
        key = per_bus = None
        if ducks is not None:
            key, per_bus = busdyn.resolve_ducks(ducks, self._mix.buses)
            for m in range(M):
                if key[m] >= 0 and owner[m] != owner[key[m]]:
                    raise ValueError("bus %d is ducked by bus %d of another launch group (class, geometry or bandwidth "
                                     "differ): a duck and its key lie in one group" % (m, key[m]))
        lengths = tuple(int(g[4]) for g in groups)
        name = (M, ch_out, lengths)
        ent = self._busdyn_handles.get(name)
        if ent is None or ent[0] is not self._busdyn:
            made = []
            for A in lengths:
                L, c, k = limiter.discretise(A)
                tables = ()
                if key is not None:
                    per = [d.discretise(A, L) if d is not None else (np.float32(1.0), np.float32(0.0), 0) for d in per_bus]
                    tables = (key, [p[0] for p in per], [p[1] for p in per], [p[2] for p in per])
                made.append((L, busdyn.create(M, ch_out, L, A, c, k, *tables)))
            ent = self._busdyn_handles.put(name, (self._busdyn, made), self._state_fence)
            for other in [shape for shape in self._busdyn_handles if shape != name]:
                del self._busdyn_handles[other]    # one shape at a time
        return [(L, h.value) for L, h in ent[1]]

    def _busdyn_group(self, L, h, mixed):
        # behind the group's rcfm_mix_run on the same stream: (processed rows, the mixer's active, bus_open_out)
        out, active, bus_open = mixed
        t = self._torch
        wet = hip.empty(tuple(out.shape), t.float32)
        open_out = hip.empty((int(out.shape[0]),), t.uint8)
        hip.check(self._lib.rcfm_busdyn_run(h, int(out.shape[1]), hip.ptr(out), hip.ptr(bus_open), hip.ptr(wet), hip.ptr(open_out),
                                            hip.stream()))
        return wet, active, open_out

    def bus_delay(self):
        """The delay of the buses in samples, one figure per launch group of this tuner's last run: the limiter's block
        length L at that group's audio rate, 0 without bus dynamics."""
        if self._last.mix is None:
            raise RuntimeError("bus_delay: no run_all / run_each with a mixer set (set_mix) yet")
        if self._last.dry is None:
            return [0] * len(self._last.mix[1])
        return [g[3] for g in self._last.dry[1]]

    def _gates(self, handle, first, count, audio):
        """What follows a group's rcfm_pipeline_run on the same stream: the tone bank, the audio filter, the level squelch
        or the frame gate, the tone squelch, each only when set.  (tones (P, E) or None, open mask or None, frame mask or None)."""
        tones = mask = frames = None
        if self._tones is not None:
            tones = self._tones[0].run(audio, step=int(audio.shape[2]), offset=0)
        if self._afilt is not None:
            self._filter_group(first, count, audio)
        if self._squelch is not None:
            mask = self._squelch_group(handle, first, count, audio)
        elif self._gate is not None:
            mask, frames = self._gate_group(handle, first, count, audio)
        if tones is not None and self._tones[1] is not None:
            mask = self._tone_squelch(first, count, audio, tones, mask)
        return tones, mask, frames

    def _squelch_group(self, handle, first, count, audio):
        # behind the group's rcfm_pipeline_run on the same stream: levels of its channels, then mask + zero fill
        def upload():
            a = self._squelch
            if a.ndim == 1 and a.shape[0] != len(self._bounds):
                raise ValueError("squelch thresholds were set for %d channels, the tuner has %d"
                                 % (a.shape[0], len(self._bounds)))
            full = np.ascontiguousarray(np.broadcast_to(a, (len(self._bounds),)))
            return hip.to_device(full, self._torch.float32)
        if isinstance(self._squelch, OverFloor):
            thr = self._floor_thresholds(self._squelch.db)
        else:
            thr = self._derived("squelch", self._squelch, self._version, upload)
        power = hip.empty((count,), self._torch.float32)
        mask = hip.empty((count,), self._torch.uint8)
        s = hip.stream()
        hip.check(self._lib.rcfm_tuner_levels(handle, first, count, hip.ptr(power), s))
        hip.check(self._lib.rcfm_squelch(hip.ptr(power), ctypes.c_void_p(thr.data_ptr() + 4 * first), count,
                                         audio.numel() // count, hip.ptr(audio), hip.ptr(mask), s))
        return mask

    def _launch_plan(self):
        """Groups of consecutive channels that share demodulator class, geometry and bandwidth, for the declared
        shard: [(first, count, kind, B, A, tau)], built once per channel-list version (O(C)) -- the steady
        state of run_all / run_each does no per-channel Python work.  Replacing ``channel.demodulator`` by hand
        after add_channel is not seen until the next add_channel / reset / shard (the reference has no such
        cache because it has no batched call)."""
        key = (self._version, self._shard)
        if self._plan is None or self._plan[0] != key:
            first, count = self._shard if self._shard is not None else (0, len(self._bounds))
            groups = []
            i = first
            while i < first + count:
                g = self._geometry(self._bounds[i].demodulator)
                bw = int(self._bounds[i].bandwidth)
                j = i + 1
                while g is not None and j < first + count and int(self._bounds[j].bandwidth) == bw and \
                        self._geometry(self._bounds[j].demodulator) == g:
                    j += 1
                groups.append((i, j - i) + (g if g is not None else (None, None, None, None)))     # (+ the AGC setting, if any)
                i = j
            self._plan = (key, groups, first, count)
        return self._plan[1], self._plan[2], self._plan[3]

    def run_all(self, numpy_output: bool = True, chunk: int = 0):
        """Audio of every channel, [C, A, ch] float32, in channel-index order.

        All channels must carry demodulators of one class and geometry.  The
        de-emphasis state is ONE per channel, carried from buffer to buffer and
        shared with the channel's demodulator object (``_bind_states``), so
        ``ch.demodulator.run(tuner.run(i))`` and this call may alternate.

        After ``shard(first, count)`` only that range is run (its spectrum rows are all ``load``
        kept) and the result is [count, A, ch] -- the block sharding.gather_audio expects.
        """
        return self._out(self._run_all_device(chunk).blocks[0][2], numpy_output)

    def _run_all_device(self, chunk=0):
        # run_all's launches on the current stream: ONE group, the shard's range (launched even when empty) with the geometry
        # all channels share; the _Run they fill (Lanes collects it later)
        handle = self._ready()
        _, first, count = self._launch_plan()
        geo = self._plan_uniform()     # ALL channels of the tuner, not only the shard's
        if geo is None:
            raise ValueError("run_all needs one demodulator class and geometry for all channels")
        return self._run_groups(handle, [(first, count) + geo], chunk)

    def _run_groups(self, handle, groups, chunk=0):
        """The launches of run_all / run_each on the current stream: per group (first, count, kind, B, A, tau[, agc]) of like
        channels its audio, rcfm_pipeline_run and what follows it (_gates); a tone bank or filter that does not fit is refused
        before the first launch.  Returns the _Run and keeps its masks and tone powers for open_mask() / tone_power()."""
        self._fit_tones(self._tones)
        self._fit_afilt(self._afilt)
        self._fit_gate(self._gate)
        owner, mixes = self._fit_mix(tuple((g[0], g[1]) for g in groups)) if self._mix is not None else (None, None)
        dynamics = self._fit_busdyn(owner, groups) if mixes is not None and self._busdyn is not None else None
        gated = self._squelch is not None or self._gate is not None or (self._tones is not None and self._tones[1] is not None)
        run = _Run([], [] if gated else None, [] if self._tones is not None else None, [] if self._gate is not None else None,
                   (owner, []) if mixes is not None else None, (owner, []) if dynamics is not None else None)
        for k, (first, count, kind, B, A, tau, *agc) in enumerate(groups):
            ch = 2 if kind == hip.RCFM_WBFM else 1
            audio = hip.empty((count, A, ch), self._torch.float32)
            hip.check(self._lib.rcfm_pipeline_run(handle, self._batched_demod(kind, B, A, tau, chunk, *agc), first, count,
                                                  hip.ptr(audio), hip.stream()))
            run.blocks.append((count, ch, audio))
            if not count:                  # run_all of an empty shard: nothing to gate, and nothing to ask for afterwards
                run = run._replace(masks=None, tones=None, frames=None)
                continue
            tones, mask, frames = self._gates(handle, first, count, audio)
            if run.masks is not None:
                run.masks.append(mask)
            if run.tones is not None:
                run.tones.append(tones)
            if run.frames is not None:
                run.frames.append(frames)
            if run.mix is not None:
                mixed = self._mix_group(mixes[k], first, count, audio, mask)
                if run.dry is not None:
                    run.dry[1].append(mixed + (dynamics[k][0],))
                    mixed = self._busdyn_group(*dynamics[k], mixed)
                run.mix[1].append(mixed)
        self._last = _Run(None, run.masks, run.tones, run.frames, run.mix, run.dry)
        return run

    def run_all_packed(self, pcm, numpy_output: bool = True, chunk: int = 0, drain=None, buses: bool = False):
        """``run_all`` for a publisher (rcfm_audio_pack; no reference counterpart): the audio of the OPEN channels only,
        packed densely in channel order in the sample format of ``pcm`` (a ``radiocore.PCM``: int16 at a gain, or float32
        unchanged).  The launches of ``run_all`` run unchanged -- squelch included when set, and ``open_mask()`` keeps
        working; with squelch off every channel is open -- and the pack follows them on the same stream.

        Without ``drain``: ``(index int32 [n_open], audio [n_open, A, ch])`` as numpy arrays, row k being channel
        ``index[k]`` of the run's range; only the n_open rows are copied to the host.  On a ``cuda=True`` tuner
        ``numpy_output=False`` returns the device tensors ``(index [count], packed [count, A, ch], n_open [1])`` without
        synchronising; entries and rows from n_open on are not written.
        With ``drain`` (a ``radiocore.tools.Drain`` of at least ``count`` rows of [A, ch] in pcm's dtype): the packed audio
        goes into the drain's next free slot and its header's copy is queued; the call returns nothing and does not
        wait -- ``drain.next()`` hands the buffer out.  RuntimeError when every slot of the drain is in flight, ValueError
        for a drain of another geometry: both before anything is launched.
        ``buses=True`` (with a mixer set, ``set_mix``): the same for the bus rows instead of the channel rows -- the M buses
        of [A, ch_out], a bus being open when one of its channels is; ``index`` then counts buses, and a drain holds at
        least M rows of [A, ch_out].  ValueError without a mixer."""
        self._ready()
        count, geo = self._launch_plan()[2], self._plan_uniform()
        if count < 1:
            raise ValueError("run_all_packed needs at least one channel")
        if buses:
            if self._mix is None:
                raise ValueError("run_all_packed(buses=True) needs a mixer (set_mix)")
            count = self._mix.M
        if drain is not None and geo is not None:          # refused before anything runs (a run advances the de-emphasis state)
            shape = (geo[2], self._mix.ch_out) if buses else (geo[2], 2 if geo[0] == hip.RCFM_WBFM else 1)
            if drain.rows < count or drain.row_shape != shape or drain.dtype != pcm.dtype:
                raise ValueError("the drain holds %d rows of %s %s, this run packs %d rows of %s %s"
                                 % (drain.rows, drain.row_shape, drain.dtype, count, shape, pcm.dtype))
        if drain is not None:
            packed, index, n_open = drain._begin()         # ... and so is a drain with every slot in flight
        run = self._run_all_device(chunk)
        if buses:
            audio, _, mask = run.mix[1][0]
        else:
            audio = run.blocks[0][2]
            mask = run.masks[0] if run.masks else None
        row = int(audio.shape[1]) * int(audio.shape[2])
        args = (hip.ptr(audio), hip.ptr(mask) if mask is not None else None, count, row, pcm.format, pcm.gain)
        if drain is not None:
            hip.check(self._lib.rcfm_audio_pack(*args, packed, index, n_open, hip.stream()))
            drain._submit()
            return None
        t = self._torch
        packed = hip.empty(tuple(audio.shape), t.int16 if pcm.format == hip.RCFM_PCM_S16 else t.float32)
        index = hip.empty((count,), t.int32)
        n_open = hip.empty((1,), t.int32)
        hip.check(self._lib.rcfm_audio_pack(*args, hip.ptr(packed), hip.ptr(index), hip.ptr(n_open), hip.stream()))
        if self._cuda and not numpy_output:
            return index, packed, n_open
        n = int(hip.to_host(n_open)[0])
        return hip.to_host(index[:n]), hip.to_host(packed[:n])

    def _plan_uniform(self):
        """(kind, B, A, tau) -- plus the AGC setting where there is one -- when every channel of the tuner carries the
        same demodulator class and geometry, else None; cached per channel-list version."""
        if self._uniform[0] != self._version:
            geo = {self._geometry(c.demodulator) for c in self._bounds}
            self._uniform = (self._version, next(iter(geo)) if len(geo) == 1 and None not in geo else None)
        return self._uniform[1]

    def run_each(self, numpy_output: bool = True):
        """What the reference's loop collects (examples/multi_fm_server.py:100-106,
        ``[ch.demodulator.run(tuner.run(ch.index)) for ch in tuner.channels()]``): a list with one audio array per
        channel, shaped as the reference's demodulators return it: [A, 1] for FM / MFM, [1, A, 2] for WBFM (wbfm.py:94 dstack) -- the shapes of FM.run / MFM.run / WBFM.run here.

        The channels may differ in demodulator class, bandwidth and audio rate (broadcast stations next to
        narrow-band ones): consecutive channels of one class and geometry run as one batched sequence, and the
        de-emphasis state is the tuner's, per channel, as in ``run_all``.  After ``shard(first, count)`` the list
        covers that range only.
        """
        return self._each_result(self._run_each_device().blocks, self._cuda and not numpy_output)

    def _run_each_device(self):
        # run_each's launches on the current stream: the launch plan's groups of like channels; the _Run they fill
        handle = self._ready()
        groups, first, count = self._launch_plan()
        if any(g[2] is None for g in groups):
            raise ValueError("run_each needs an FM, MFM, WBFM, AM, USB or LSB demodulator on every channel")
        return self._run_groups(handle, groups)

    def _each_result(self, blocks, device_output):
        out = []
        for n, ch, audio in blocks:
            block = self._result(audio, device_output)
            out.extend(block[k:k + 1] if ch == 2 else block[k] for k in range(n))
        return out

    @staticmethod
    def _geometry(demod):
        kind = _KINDS.get(type(demod).__name__)
        if kind is None:
            return None
        geo = (kind, demod._input_size, demod._output_size, demod._tau)
        agc = getattr(demod, "_agc", None)          # (decay_samples, level, floor); off: the four-tuple as ever
        return geo if agc is None else geo + (agc,)

    def reset_states(self):
        """Every channel's de-emphasis state back to the reference's freshly constructed filters (deemphasis.py:48-49),
        and every AGC back to "no history": the batched handles of run_all / run_each, whose slots the channels'
        demodulator objects share.  The audio filter's states (set_audio_filter) go back to rest as well, and the frame
        gate (set_gate) closes every channel."""
        for h in self._batched.values():
            hip.check(self._lib.rcfm_demod_reset_state(h.value, hip.stream()))
        for cache in self._carried.values():
            cache.reset_states()

    def set_kernel_options(self, lds_chain=True, fused_tiles=True, phase_link=True, narrow_tiles=1, ssb_direct=True):
        """Which forms of the kernel chain run_all / run_each may use (rcfm_demod_set_option; no reference
        counterpart).  The audio does not depend on them beyond float32 rounding: switching all three off gives a
        second evaluation of the same path that shares no kernel schedule with the default one, which is what the
        full-size parity tests compare against.  narrow_tiles: 0 = tile kernels with 16 lines per tile always, 1 = 8 lines
        when a launch has fewer than two tiles per CU (the default), 2 = always 8.  ssb_direct: USB / LSB audio straight
        from the loaded spectrum (False: through channel samples, RCFM_OPT_SSB_DIRECT).  Takes effect with the next
        run_all / run_each."""
        self._kernel_options = (bool(lds_chain), bool(fused_tiles), bool(phase_link), int(narrow_tiles), bool(ssb_direct))

    def _batched_demod(self, kind, B, A, tau, chunk, agc=None):
        # one handle per geometry (and AGC setting), sized for all channels: rcfm_pipeline_run addresses the channels of
        # tuner and demodulator by the same index, so the per-channel state survives regrouping
        opts = self._kernel_options
        key = (kind, len(self._bounds), B, A, tau, int(chunk)) + ((opts,) if opts != _DEFAULT_OPTIONS else ())
        if agc is not None:
            key += (("agc", agc),)
        if key not in self._batched:
            h = ctypes.c_void_p()
            with hip.bound(self._arena):
                hip.check(self._lib.rcfm_demod_create(kind, len(self._bounds), B, A, tau, int(chunk), ctypes.byref(h)))
            self._batched[key] = hip.Handle(h, self._lib.rcfm_demod_destroy)
            if agc is not None:                   # before the binding: set_agc gives the handle a state of its own
                hip.check(self._lib.rcfm_demod_set_agc(h, *agc))
            for opt, on in zip((hip.RCFM_OPT_LDS_CHAIN, hip.RCFM_OPT_FUSED_TILES, hip.RCFM_OPT_PHASE_LINK), opts[:3]):
                if not on:
                    hip.check(self._lib.rcfm_demod_set_option(h, opt, 0))
            if not opts[4]:
                hip.check(self._lib.rcfm_demod_set_option(h, hip.RCFM_OPT_SSB_DIRECT, 0))
            if opts[3] != 1:   # (rcfm_pipeline_run hands the same setting to the tuner's inverse FFT of each chunk)
                hip.check(self._lib.rcfm_demod_set_option(h, hip.RCFM_OPT_NARROW_TILES, opts[3]))
            self._bind_states(key, self._batched[key])
            if self._state_fence and (kind not in _STATELESS or agc is not None):    # after the binding: the fence travels with the state buffer
                hip.check(self._lib.rcfm_demod_set_option(h, hip.RCFM_OPT_STATE_FENCE, 1))
        elif self._bound_version.get(key) != self._version:
            self._bind_states(key, self._batched[key])
        return self._batched[key].value

    def _bind_states(self, key, handle):
        """ONE de-emphasis state per channel, as in the reference, where it lives in the demodulator object the
        Channel carries (deemphasis.py:48-49,64; wbfm.py:53-57): every channel's demodulator instance of this
        geometry keeps its state in its channel's slot of the batched handle from now on (rcfm_demod_bind_state moves
        what it has carried so far), and further batched handles of the same geometry (another `chunk`) share the
        first one's buffer.  Mixing ``ch.demodulator.run(tuner.run(i))`` and ``run_all()`` across buffers then gives
        what the reference's loop gives.  O(C) Python, once per change of the channel list; a demodulator whose own
        librcfm handle does not exist yet (it is created on first use) binds when it does; FM, AM, USB and LSB carry no
        state -- unless AM / USB / LSB run an AGC, whose follower is bound the same way, per AGC setting."""
        kind, C, B, A, tau = key[:5]
        agc = _key_agc(key)
        self._bound_version[key] = self._version
        if kind in _STATELESS and agc is None:
            return
        owner_key = (kind, C, B, A, tau) + ((agc,) if agc is not None else ())
        owner = self._state_owner.get(owner_key)
        if owner is None:
            self._state_owner[owner_key] = handle
        elif owner.value != handle.value:
            hip.check(self._lib.rcfm_demod_bind_state(handle.value, owner.value, 0, 0, hip.stream()))   # the owner has the history
        if self._is_lane:
            return                          # the channels' demodulator objects stay bound to the base tuner's handle
        geo = (kind, B, A, tau) + ((agc,) if agc is not None else ())
        seen = set()
        for c in self._bounds:
            d = c.demodulator
            if id(d) in seen or self._geometry(d) != geo or getattr(d, "_batch", 0) != 1:
                continue                      # (an object registered on two channels keeps its first slot)
            seen.add(id(d))
            d._bind(handle, c.index)

    # ---- consecutive buffers on several streams (radiocore.tools.Lanes) ---------------------------------------------

    def _arm_state_fence(self):
        """From now on this tuner's batched demodulator handles may be used from several streams: every launch sequence
        that touches the shared de-emphasis state waits for the previous one (rcfm_demod_set_option, RCFM_OPT_STATE_FENCE)."""
        self._state_fence = True
        for key, h in self._batched.items():
            if key[0] not in _STATELESS or _key_agc(key) is not None:
                hip.check(self._lib.rcfm_demod_set_option(h.value, hip.RCFM_OPT_STATE_FENCE, 1))
        for cache in self._carried.values():
            cache.arm()

    def _lane_clone(self):
        """A second Tuner over the SAME channel list, demodulator objects and de-emphasis state, with its own device
        handles (spectrum, workspaces): what one more stream needs to work on the next buffer."""
        t = Tuner(cuda=self._cuda)
        t._arena = self._arena
        t._is_lane = True
        t._state_fence = True
        t._state_owner = self._state_owner        # shared, the same dicts: one de-emphasis state per channel, whoever runs it ...
        t._carried = self._carried                # ... and one of every carried state, under the same names;
        t.__dict__.update(self._carried)          # every other device handle is the lane's own
        t._sync_lane(self)
        return t

    def _sync_lane(self, base):
        """Follow the base tuner: its settings, each a new object per set_* -- what this lane made from the old one is made
        again when it is next used (_derived), on the lane's own stream -- and its channel list."""
        drops = {drop for name, drop in _FOLLOWED.items() if getattr(self, name) is not getattr(base, name)}
        if "last" in drops:
            self._last = _Run()                            # (Lanes keeps each buffer's results with its ticket)
        if "blanker" in drops:
            self.set_blanker(None)                         # the handle and scratch of this lane's own go with their blanker
        if "floor" in drops:
            self._floor_out = None                         # (the handles are shared: the base tuner's set_floor dropped them)
        for name in _FOLLOWED:
            setattr(self, name, getattr(base, name))
        if self._version == base._version and self._bounds is base._bounds and self._shard == base._shard and \
                self._input_bandwidth == base._input_bandwidth:
            return
        self._bounds = base._bounds
        self._input_frequency, self._input_bandwidth = base._input_frequency, base._input_bandwidth
        self._lo, self._hi, self._bw_sum = base._lo, base._hi, base._bw_sum
        self._version = base._version
        self._win_size = base._win_size
        self._kernel_options = base._kernel_options
        if base._shard is not None and self._shard != base._shard:
            self.shard(*base._shard)
