"""Python host side of the batched RXA engine (include/quiskhip.h group 1).

Method names are the WDSP export names the reference binds through ctypes
(quisk_wdsp.py:79-91, quisk.py:6017-6052); the first argument is the channel index inside the
batch, or -1 for all channels.
"""
import ctypes as C

import numpy as np

from .lib import load, check, QuiskHipError

_SETTERS = ("SetRXAMode", "RXASetNC", "SetRXAShiftRun", "RXANBPSetRun", "SetRXABandpassRun", "SetRXAAGCMode",
            "SetRXAPanelSelect", "SetRXAPanelCopy", "SetRXAShiftFreq", "SetRXAAGCFixed", "SetRXAPanelGain1",
            "RXASetPassband", "RXANBPSetFreqs", "SetRXABandpassFreqs", "SetRXAPanelGain2", "SetRXAAMDSBMode",
            "SetRXAAMDFadeLevel", "SetRXAFMDeviation", "SetRXACTCSSFreq", "SetRXACTCSSRun", "SetRXAAGCAttack",
            "SetRXAAGCDecay", "SetRXAAGCHang", "SetRXAAGCTop", "SetRXAAGCSlope", "SetRXAAGCHangThreshold", "RXASetMP",
            "SetRXAAMDRun", "RXANBPSetNotchesRun", "RXANBPSetWindow", "RXANBPSetAutoIncrease", "RXANBPSetTuneFrequency",
            "RXANBPSetShiftFrequency", "SetRXAFMLimRun", "SetRXAFMLimGain",
            "SetRXASNBARun", "SetRXASNBAOutputBandwidth", "SetRXASNBAasize", "SetRXASNBAnpasses", "SetRXASNBAk1", "SetRXASNBAk2", "SetRXASNBAbridge", "SetRXASNBApresamps", "SetRXASNBApostsamps", "SetRXASNBApmultmin", "SetRXASNBAovrlp", "SetRXAEMNRRun", "SetRXAEMNRgainMethod", "SetRXAEMNRnpeMethod", "SetRXAEMNRaeRun", "SetRXAEMNRPosition", "SetRXAEMNRaeZetaThresh", "SetRXAEMNRaePsi", "SetRXAEMNRtrainZetaThresh", "SetRXAEMNRtrainT2",
            "SetRXAAMSQRun", "SetRXAAMSQThreshold", "SetRXAAMSQMaxTail", "SetRXAANFRun", "SetRXAANFTaps", "SetRXAANFDelay", "SetRXAANFPosition", "SetRXAANFGain", "SetRXAANFLeakage", "SetRXAANFVals",
            "SetRXAANRRun", "SetRXAANRTaps", "SetRXAANRDelay", "SetRXAANRPosition", "SetRXAANRGain", "SetRXAANRLeakage", "SetRXAANRVals",
            "SetRXACBLRun", "SetRXASPCWRun", "SetRXASPCWFreq", "SetRXASPCWBandwidth", "SetRXASPCWGain", "SetRXAmpeakRun",
            "SetRXAmpeakNpeaks", "SetRXAmpeakFilEnable", "SetRXAmpeakFilFreq", "SetRXAmpeakFilBw", "SetRXAmpeakFilGain",
            "SetRXASSQLRun", "SetRXASSQLThreshold", "SetRXASSQLTauMute", "SetRXASSQLTauUnMute",
            "SetRXAFMSQRun", "SetRXAFMSQThreshold", "SetRXAFMSQNC", "SetRXAFMSQMP",
            "SetRXAFMAFFilter", "SetRXAFMNCde", "SetRXAFMMPde", "SetRXAFMNCaud", "SetRXAFMMPaud",
            "SetRXAEQRun", "SetRXAEQNC", "SetRXAEQMP", "SetRXAEQProfile", "SetRXAEQCtfmode", "SetRXAEQWintype", "SetRXAGrphEQ", "SetRXAGrphEQ10",
            "SetRXAAGCThresh", "SetRXAAGCHangLevel", "SetRXAAGCMaxInputLevel", "SetRXAPanelPan", "SetRXAPanelBinaural",
            "RXANBPSetNC", "RXANBPSetMP", "RXABPSNBASetNC", "RXABPSNBASetMP", "SetRXABandpassNC", "SetRXABandpassMP", "SetRXABandpassWindow")
# the setters that take arrays: (element type, position among the arguments behind the channel)
_ARRAYS = {"SetRXAEQProfile": ((C.c_double, 1), (C.c_double, 2)), "SetRXAGrphEQ": ((C.c_int, 0),), "SetRXAGrphEQ10": ((C.c_int, 0),)}


class AudioFormat(C.Structure):
    """qh_audio_format (include/quiskhip.h 7b): the narrowing of Quisk's sound back ends (sound_alsa.c:344-390,
    sound_pulseaudio.c:684-695).  kind: "i16", "i24", "i32", "f32"."""
    _fields_ = [("kind", C.c_int), ("num_channels", C.c_int), ("channel_I", C.c_int), ("channel_Q", C.c_int),
                ("volume", C.c_double), ("prescale", C.c_double)]
    KINDS = {"i16": 1, "i24": 2, "i32": 3, "f32": 4}
    NP = {1: np.int16, 2: np.uint8, 3: np.int32, 4: np.float32}

    def __init__(self, kind="i16", volume=1.0, prescale=1.0, num_channels=2, channel_I=0, channel_Q=1):
        super().__init__(self.KINDS[kind], num_channels, channel_I, channel_Q, volume, prescale)

    @property
    def frame_bytes(self):
        return self.num_channels * (2 if self.kind == 1 else 3 if self.kind == 2 else 4)


class RxaEngine:
    """nch independent WDSP-RXA receiver channels on one MI355X."""

    def __init__(self, nch, dsp_size=256, in_rate=192000, dsp_rate=48000, out_rate=48000, device=0, stream=None):
        self._L = load()
        self._h = self._L.qh_rxa_create(device, nch, dsp_size, in_rate, dsp_rate, out_rate, stream)
        if not self._h:
            raise QuiskHipError("qh_rxa_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch = nch
        self.dsp_insize = self._L.qh_rxa_dsp_insize(self._h)
        self.dsp_outsize = self._L.qh_rxa_dsp_outsize(self._h)
        self._emnr = None

    def load_emnr_tables(self, path=None):
        """EMNR's gain tables (WDSP's `calculus` / `zetaHat.bin` data, extracted by tools/extract_wdsp_emnr_tables.py)."""
        import os
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "wdsp_emnr_tables.npz")
        z = np.load(path)
        t = [np.ascontiguousarray(z["GG"], dtype=np.float64), np.ascontiguousarray(z["GGS"], dtype=np.float64),
             np.ascontiguousarray(z["zeta_hat"], dtype=np.float64), np.ascontiguousarray(z["zeta_valid"], dtype=np.int32)]
        r = [float(v) for v in z["zeta_range"]]
        check(self._L.qh_rxa_SetEMNRTables(self._h, t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data, t[3].ctypes.data, *r))
        self._emnr = t

    def __getattr__(self, name):
        if name in _SETTERS:
            f = getattr(self._L, "qh_rxa_" + name)

            def call(ch, *args):
                args = list(args)
                for t, pos in _ARRAYS.get(name, ()):        # sequences -> C arrays (None stays a null pointer)
                    if args[pos] is not None:
                        args[pos] = (t * len(args[pos]))(*args[pos])
                check(f(self._h, ch, *args))
            return call
        raise AttributeError(name)

    # the notch database (wdsp/nbp.c:358-469): results are the reference's return values (0 / -1)
    def RXANBPAddNotch(self, ch, notch, fcenter, fwidth, active):
        r = C.c_int(-1)
        check(self._L.qh_rxa_RXANBPAddNotch(self._h, ch, notch, fcenter, fwidth, active, C.byref(r)))
        return r.value

    def RXANBPEditNotch(self, ch, notch, fcenter, fwidth, active):
        r = C.c_int(-1)
        check(self._L.qh_rxa_RXANBPEditNotch(self._h, ch, notch, fcenter, fwidth, active, C.byref(r)))
        return r.value

    def RXANBPDeleteNotch(self, ch, notch):
        r = C.c_int(-1)
        check(self._L.qh_rxa_RXANBPDeleteNotch(self._h, ch, notch, C.byref(r)))
        return r.value

    def RXANBPGetNotch(self, ch, notch):
        f, w, a, r = C.c_double(0), C.c_double(0), C.c_int(0), C.c_int(-1)
        check(self._L.qh_rxa_RXANBPGetNotch(self._h, ch, notch, C.byref(f), C.byref(w), C.byref(a), C.byref(r)))
        return r.value, f.value, w.value, a.value

    def RXANBPGetNumNotches(self, ch):
        n = C.c_int(0)
        check(self._L.qh_rxa_RXANBPGetNumNotches(self._h, ch, C.byref(n)))
        return n.value

    def RXANBPGetMinNotchWidth(self, ch):
        w = C.c_double(0)
        check(self._L.qh_rxa_RXANBPGetMinNotchWidth(self._h, ch, C.byref(w)))
        return w.value

    # the AGC's display-side getters (wdsp/wcpAGC.c:440-520): host arithmetic on the channel's settings, nothing on the device is waited for
    def GetRXAAGCThresh(self, ch, size, rate):
        v = C.c_double(0)
        check(self._L.qh_rxa_GetRXAAGCThresh(self._h, ch, C.byref(v), float(size), float(rate)))
        return v.value

    def GetRXAAGCHangLevel(self, ch):
        v = C.c_double(0)
        check(self._L.qh_rxa_GetRXAAGCHangLevel(self._h, ch, C.byref(v)))
        return v.value

    def GetRXAAGCHangThreshold(self, ch):
        v = C.c_int(0)
        check(self._L.qh_rxa_GetRXAAGCHangThreshold(self._h, ch, C.byref(v)))
        return v.value

    def GetRXAAGCTop(self, ch):
        v = C.c_double(0)
        check(self._L.qh_rxa_GetRXAAGCTop(self._h, ch, C.byref(v)))
        return v.value

    def process_ptr(self, d_in, in_stride, d_out, out_stride, nblk):
        """Device pointers (ints), strides in complex samples.  Asynchronous on the engine's stream."""
        check(self._L.qh_rxa_process(self._h, d_in, in_stride, d_out, out_stride, nblk))

    def process_host(self, x):
        """x: complex128 [nch, nblk*dsp_insize] on the host -> complex128 [nch, nblk*dsp_outsize]."""
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] != self.nch or x.shape[1] % self.dsp_insize:
            raise ValueError("expected [nch, k*dsp_insize] complex128")
        nblk = x.shape[1] // self.dsp_insize
        out = np.empty((self.nch, nblk * self.dsp_outsize), dtype=np.complex128)
        check(self._L.qh_rxa_process_host(self._h, x.ctypes.data, x.shape[1], out.ctypes.data, out.shape[1], nblk))
        return out

    def process_audio_ptr(self, d_in, in_stride, d_out, out_stride_bytes, nblk, fmt):
        """Like process_ptr, the output as audio frames (AudioFormat) narrowed in the last kernel's store."""
        check(self._L.qh_rxa_process_audio(self._h, d_in, in_stride, d_out, out_stride_bytes, nblk, C.byref(fmt)))

    def process_packed_ptr(self, d_src, src_bytes, fmt, chan_stride, d_out, out_stride, nblk):
        """Wire-format input (quisk_amd.ingest.IqFormat) decoded inside the first kernel's load."""
        check(self._L.qh_rxa_process_packed(self._h, d_src, src_bytes, C.byref(fmt), chan_stride, d_out, out_stride, nblk))

    def process_packed_host(self, buf, fmt, chan_stride, nblk):
        raw = np.frombuffer(bytes(buf), dtype=np.uint8)
        out = np.empty((self.nch, nblk * self.dsp_outsize), dtype=np.complex128)
        check(self._L.qh_rxa_process_packed_host(self._h, raw.ctypes.data, raw.size, C.byref(fmt), chan_stride, out.ctypes.data,
                                                 out.shape[1], nblk))
        return out

    def enable_meters(self, on=True):
        check(self._L.qh_rxa_enable_meters(self._h, 1 if on else 0))

    def GetRXAMeter(self, ch, mt):
        v = C.c_double(0)
        check(self._L.qh_rxa_GetRXAMeter(self._h, ch, mt, C.byref(v)))
        return v.value

    # the data taps (wdsp/sender.c, wdsp/siphon.c): off until enabled, ch -1 = every channel
    def set_sender(self, ch, run=True):
        """xsender (RXA.c:570): later calls leave channel ch's signal behind nbp0 as float pairs on the device"""
        check(self._L.qh_rxa_set_sender(self._h, ch, 1 if run else 0))

    def sender_rows_ptr(self):
        """(device pointer, row stride in float pairs, samples per row) of the last call's sender rows"""
        p, s, n = C.c_void_p(), C.c_longlong(0), C.c_int(0)
        check(self._L.qh_rxa_sender_rows(self._h, C.byref(p), C.byref(s), C.byref(n)))
        return p.value, s.value, n.value

    def sender_rows_host(self, ch):
        """complex64 [n]: the last call's sender row of channel ch (I + jQ, the chain's order)"""
        _, _, n = self.sender_rows_ptr()
        out = np.zeros(max(n, 1), dtype=np.complex64)
        got = C.c_int(0)
        check(self._L.qh_rxa_sender_rows_host(self._h, ch, out.ctypes.data, out.size, C.byref(got)))
        return out[:got.value]

    def set_siphon(self, ch, run=True):
        """xsiphon (RXA.c:590): later calls keep the newest 4096 samples of channel ch's audio behind the AGC"""
        check(self._L.qh_rxa_set_siphon(self._h, ch, 1 if run else 0))

    def get_sip(self, ch, size):
        """complex128 [size]: the newest `size` samples of channel ch's siphon, oldest first (suck, siphon.c:148-163)"""
        out = np.zeros(max(int(size), 0), dtype=np.complex128)
        check(self._L.qh_rxa_get_sip(self._h, ch, out.ctypes.data if out.size else np.zeros(1, dtype=np.complex128).ctypes.data, int(size)))
        return out

    def attach_display(self, bank, ss=0):
        """Every later process call ends by feeding its sender rows to sub-span ss of an AnalyzerBank with a display per channel
        (None detaches).  The bank is kept alive while it is attached."""
        check(self._L.qh_rxa_attach_display(self._h, bank._h if bank is not None else None, ss))
        self._display = bank

    # gen0, the signal generator at the head of the chain (wdsp/gen.c:384-450): ch -1 = every channel
    def SetRXAPreGenRun(self, ch, run):
        """a running generator replaces the channel's signal behind the front stage (RXA.c:565)"""
        check(self._L.qh_rxa_SetRXAPreGenRun(self._h, ch, 1 if run else 0))

    def SetRXAPreGenMode(self, ch, mode):
        """0 tone, 1 two-tone, 2 noise, 3 sweep, 6 pulse, any other silence; 4 and 5 are refused at the next call"""
        check(self._L.qh_rxa_SetRXAPreGenMode(self._h, ch, int(mode)))

    def SetRXAPreGenToneMag(self, ch, mag):
        check(self._L.qh_rxa_SetRXAPreGenToneMag(self._h, ch, float(mag)))

    def SetRXAPreGenToneFreq(self, ch, freq):
        check(self._L.qh_rxa_SetRXAPreGenToneFreq(self._h, ch, float(freq)))

    def SetRXAPreGenNoiseMag(self, ch, mag):
        check(self._L.qh_rxa_SetRXAPreGenNoiseMag(self._h, ch, float(mag)))

    def SetRXAPreGenSweepMag(self, ch, mag):
        check(self._L.qh_rxa_SetRXAPreGenSweepMag(self._h, ch, float(mag)))

    def SetRXAPreGenSweepFreq(self, ch, freq1, freq2):
        check(self._L.qh_rxa_SetRXAPreGenSweepFreq(self._h, ch, float(freq1), float(freq2)))

    def SetRXAPreGenSweepRate(self, ch, rate):
        check(self._L.qh_rxa_SetRXAPreGenSweepRate(self._h, ch, float(rate)))

    def set_gen_seed(self, ch, seed):
        """the seed of the channel's noise stream (the default is a fixed function of the channel)"""
        check(self._L.qh_rxa_set_gen_seed(self._h, ch, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def pll_repairs(self):
        return self._L.qh_rxa_pll_repairs(self._h)

    def debug_fmsq(self, ch):
        """diagnostics: the FM squelch of channel ch at the last call's end: (avnoise, longnoise, state, count, ready), or None while no
        channel of the engine has run it"""
        buf = (C.c_double * 5)()
        n = self._L.qh_rxa_debug_fmsq(self._h, ch, buf, 5)
        check(n if n < 0 else 0)
        return (buf[0], buf[1], int(buf[2]), int(buf[3]), int(buf[4])) if n == 5 else None

    def debug_fm_rows(self):
        """diagnostics: (de-emphasis rows, audio rows, rows designed so far): the mask rows xfmd's two filters hold on the device, one per
        distinct design among the running FM channels, and how many designs the host has made since the engine was made or rebuilt"""
        de, au, n = C.c_int(0), C.c_int(0), C.c_longlong(0)
        check(self._L.qh_rxa_debug_fm_rows(self._h, C.byref(de), C.byref(au), C.byref(n)))
        return de.value, au.value, n.value

    def debug_eqp(self, ch, max_nc=4096):
        """diagnostics: the complex taps behind the mask channel ch's equalizer last got (nc of them, scale 1 / (2 dsp_size) as WDSP's
        fircore gets them; a setter's new design shows after the next process call that runs the channel's equalizer), or None while no
        channel of the engine has run the stage"""
        buf = (C.c_double * (2 * max_nc))()
        n = self._L.qh_rxa_debug_eqp(self._h, ch, buf, 2 * max_nc)
        check(n if n < 0 else 0)
        return np.frombuffer(buf, dtype=np.complex128, count=n).copy() if n > 0 else None

    def debug_agc(self, form):
        """diagnostics: 0 = time tiles for long calls (default), 1 = the sample-by-sample form of the wcpAGC loop, 2 = 64 samples per step"""
        check(self._L.qh_rxa_debug_agc(self._h, int(form)))

    def agc_repairs(self):
        return self._L.qh_rxa_agc_repairs(self._h)

    def agc_segments_rerun(self):
        return self._L.qh_rxa_agc_segments_rerun(self._h)

    def agc_tiled_channels(self):
        return self._L.qh_rxa_agc_tiled_channels(self._h)

    def synchronize(self):
        check(self._L.qh_rxa_synchronize(self._h))

    def flush(self):
        """flush_rxa (wdsp/RXA.c:537-559): every stage's state back to its start"""
        check(self._L.qh_rxa_flush(self._h))

    def set_graph_replay(self, on=True):
        """Block-at-a-time callers: replay the launch sequence of process_ptr from hipGraphs while nothing changes."""
        check(self._L.qh_rxa_set_graph_replay(self._h, 1 if on else 0))

    def set_band_tile(self, nfft=0):
        """Tile of the band-pass stages: 4096 (0 = default) or 8192 (two lane groups per tile; measured slower)."""
        check(self._L.qh_rxa_set_band_tile(self._h, int(nfft)))

    def band_tile(self):
        return self._L.qh_rxa_band_tile(self._h)

    def set_snba_form(self, form=0):
        """Form of xsnba: 0 = the single kernel where it can run (default), 1 = the three passes everywhere; the same bits."""
        check(self._L.qh_rxa_set_snba_form(self._h, int(form)))

    def snba_form(self):
        return self._L.qh_rxa_snba_form(self._h)

    def graph_launches(self):
        return self._L.qh_rxa_graph_launches(self._h)

    def enable_timing(self, on=True):
        check(self._L.qh_rxa_enable_timing(self._h, 1 if on else 0))

    def timing_ms(self):
        buf = (C.c_double * 3)()
        n = self._L.qh_rxa_timing(self._h, buf, 3)
        return [buf[k] for k in range(n)]

    def device_bytes(self):
        return self._L.qh_rxa_device_bytes(self._h)

    # the run-time rate and buffer-size setters (wdsp/channel.c:169-258; include/quiskhip.h): every per-channel setting survives
    def _resized(self, rc):
        check(rc)
        self.dsp_insize = self._L.qh_rxa_dsp_insize(self._h)
        self.dsp_outsize = self._L.qh_rxa_dsp_outsize(self._h)

    def set_rates(self, in_rate, dsp_rate, out_rate):
        self._resized(self._L.qh_rxa_set_rates(self._h, int(in_rate), int(dsp_rate), int(out_rate)))

    def set_in_rate(self, in_rate):
        self._resized(self._L.qh_rxa_set_in_rate(self._h, int(in_rate)))

    def set_dsp_rate(self, dsp_rate):
        self._resized(self._L.qh_rxa_set_dsp_rate(self._h, int(dsp_rate)))

    def set_out_rate(self, out_rate):
        self._resized(self._L.qh_rxa_set_out_rate(self._h, int(out_rate)))

    def set_dsp_size(self, dsp_size):
        self._resized(self._L.qh_rxa_set_dsp_size(self._h, int(dsp_size)))

    @property
    def in_rate(self):
        return self._L.qh_rxa_in_rate(self._h)

    @property
    def dsp_rate(self):
        return self._L.qh_rxa_dsp_rate(self._h)

    @property
    def out_rate(self):
        return self._L.qh_rxa_out_rate(self._h)

    @property
    def dsp_size(self):
        return self._L.qh_rxa_dsp_size(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_rxa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
