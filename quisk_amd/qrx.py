"""Python host side of the Quisk-native receiver bank (include/quiskhip.h group 6).

Method names follow the _quisk calls the GUI makes: set_tune (quisk.c:4702), set_filters (quisk.c:4551),
get_filter_rate (quisk.c:2787).  Rx filter taps come from quisk_amd.rxfilter.make_filter_coef, the restatement of
quisk.py's MakeFilterCoef.
"""
import ctypes as C

import numpy as np

from . import rxfilter
from .lib import load, check, QuiskHipError


_TABLE_KEYS = ("quiskFilt48dec24Coefs", "quiskFilt144D3Coefs", "quiskFilt240D5CoefsSharp", "quiskAudio24p4Coefs",
               "quiskAudio24p6Coefs", "quiskLpFilt48Coefs", "quiskAudioFmHpCoefs", "quiskFilt300D5Coefs",
               "quiskFilt53D1Coefs", "quiskFilt111D2Coefs", "quiskFilt133D2Coefs", "quiskFilt167D3Coefs",
               "quiskFilt185D3Coefs")


class _Tables(C.Structure):         # include/quiskhip.h: qh_qrx_tables
    _fields_ = [(k, C.c_void_p) for k in _TABLE_KEYS]


class QuiskRxBank:
    """`bandwidth` is what the GUI passes as set_filters' third argument (quisk.c:4581); it decides the filter
    rate of the DGT / FDV modes and whether DGT-IQ is filtered at all."""

    def __init__(self, nch, sample_rate, mode, bandwidth=2700, device=0, stream=None):
        self._L = load()
        t = rxfilter.coefficient_tables()
        self._tabs = [np.ascontiguousarray(t[k], dtype=np.float64) for k in _TABLE_KEYS]
        self._tstruct = _Tables(*[a.ctypes.data for a in self._tabs])
        self._h = self._L.qh_qrx_create_ex(device, nch, sample_rate, mode, bandwidth, C.byref(self._tstruct), stream)
        if not self._h:
            raise QuiskHipError("qh_qrx_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch, self.sample_rate, self.mode, self.bandwidth = nch, sample_rate, mode, bandwidth

    def get_decim_rate(self):
        return self._L.qh_qrx_decim_rate(self._h)

    def get_filter_rate(self):
        return self._L.qh_qrx_filter_rate(self._h)

    def set_tune(self, ch, rx_tune_freq):
        check(self._L.qh_qrx_set_tune(self._h, ch, int(rx_tune_freq)))

    def set_tune_all(self, rx_tune_freqs):
        """every receiver's set_tune (quisk.c:4702) in one launch per table: rx_tune_freqs[nch] Hz"""
        f = np.ascontiguousarray(rx_tune_freqs, dtype=np.int32)
        assert f.size == self.nch
        check(self._L.qh_qrx_set_tune_all(self._h, f.ctypes.data))

    def set_filters(self, ch, filtI, filtQ):
        fI = np.ascontiguousarray(filtI, dtype=np.float64)
        fQ = np.ascontiguousarray(filtQ, dtype=np.float64)
        if fI.size != fQ.size:
            raise ValueError("The size of filters I and Q must be equal")
        check(self._L.qh_qrx_set_filters(self._h, ch, fI.ctypes.data, fQ.ctypes.data, fI.size))

    def set_agc(self, on, release_gain=80.0):
        """process_agc on the output like quisk_process_samples; release_gain is QS.set_agc's argument (quisk.c:4543)."""
        check(self._L.qh_qrx_set_agc(self._h, 1 if on else 0, float(release_gain)))

    def set_auto_notch(self, on, rit_freq=0):
        """QS.set_auto_notch (quisk.c:4596): dAutoNotch on the demodulated audio; rit_freq keeps CW's sidetone."""
        check(self._L.qh_qrx_set_auto_notch(self._h, 1 if on else 0, int(rit_freq)))

    def set_noise_blanker(self, level):
        """QS.set_noise_blanker (quisk.c:4605): NoiseBlanker on the raw samples ahead of the tune; 0 = off."""
        check(self._L.qh_qrx_set_noise_blanker(self._h, int(level)))

    def set_ssb_squelch(self, enabled, level):
        """QS.set_ssb_squelch (quisk.c:4729): CW / SSB / AM."""
        check(self._L.qh_qrx_set_ssb_squelch(self._h, 1 if enabled else 0, int(level)))

    def set_squelch(self, ch, level):
        """FM squelch threshold, QS.set_squelch (quisk.c:4721)."""
        check(self._L.qh_qrx_set_squelch(self._h, ch, float(level)))

    def out_count(self, n_in):
        return self._L.qh_qrx_out_count(self._h, n_in)

    def process_ptr(self, d_in, in_stride, n_in, d_out, out_stride):
        n = C.c_int(0)
        check(self._L.qh_qrx_process(self._h, d_in, in_stride, n_in, d_out, out_stride, C.byref(n)))
        return n.value

    def process_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise ValueError("expected [nch, n] complex128")
        cap = max(self.out_count(x.shape[1]), 1)
        out = np.empty((self.nch, cap), dtype=np.complex128)
        n = C.c_int(0)
        check(self._L.qh_qrx_process_host(self._h, x.ctypes.data, x.shape[1], x.shape[1], out.ctypes.data, cap, C.byref(n)))
        return out[:, :n.value].copy()

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_qrx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuiskProcessBank:
    """quisk_process_samples (quisk.c:2289-2742) for a bank of receivers (include/quiskhip.h group 9b): test tone / inversion,
    NoiseBlanker, the panadapter's feed, tune + decimate + demodulate, cFracDecim, interpolation to the playback rate, process_agc
    (always on, as in the reference) and the squelches.  Method names follow the _quisk calls."""

    def __init__(self, nch, sample_rate, mode, bandwidth=2700, playback_rate=48000, fft_size=0, data_width=0, device=0, stream=None):
        self._L = load()
        t = rxfilter.coefficient_tables()
        self._tabs = [np.ascontiguousarray(t[k], dtype=np.float64) for k in _TABLE_KEYS]
        self._tstruct = _Tables(*[a.ctypes.data for a in self._tabs])
        self._h = self._L.qh_qps_create(device, nch, sample_rate, playback_rate, mode, bandwidth, C.byref(self._tstruct), fft_size, data_width, stream)
        if not self._h:
            raise QuiskHipError("qh_qps_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch, self.sample_rate, self.mode, self.data_width = nch, sample_rate, mode, data_width

    def get_filter_rate(self):
        return self._L.qh_qps_filter_rate(self._h)

    def get_decim_rate(self):
        return self._L.qh_qps_decim_rate(self._h)

    def set_tune(self, ch, rx_tune_freq):
        check(self._L.qh_qps_set_tune(self._h, ch, int(rx_tune_freq)))

    def set_tune_all(self, rx_tune_freqs):
        """every receiver's set_tune in one launch per table: rx_tune_freqs[nch] Hz"""
        f = np.ascontiguousarray(rx_tune_freqs, dtype=np.int32)
        assert f.size == self.nch
        check(self._L.qh_qps_set_tune_all(self._h, f.ctypes.data))

    def set_filters(self, ch, filtI, filtQ):
        fI = np.ascontiguousarray(filtI, dtype=np.float64)
        fQ = np.ascontiguousarray(filtQ, dtype=np.float64)
        if fI.size != fQ.size:
            raise ValueError("The size of filters I and Q must be equal")
        check(self._L.qh_qps_set_filters(self._h, ch, fI.ctypes.data, fQ.ctypes.data, fI.size))

    def set_agc(self, level):
        check(self._L.qh_qps_set_agc(self._h, float(level)))

    def set_noise_blanker(self, level):
        check(self._L.qh_qps_set_noise_blanker(self._h, int(level)))

    def set_auto_notch(self, on, rit_freq=0):
        check(self._L.qh_qps_set_auto_notch(self._h, 1 if on else 0, int(rit_freq)))

    def invert_spectrum(self, invert):
        check(self._L.qh_qps_invert_spectrum(self._h, 1 if invert else 0))

    def set_kill_audio(self, kill):
        check(self._L.qh_qps_set_kill_audio(self._h, 1 if kill else 0))

    def add_tone(self, freq):
        check(self._L.qh_qps_add_tone(self._h, int(freq)))

    def set_squelch(self, ch, level):
        check(self._L.qh_qps_set_squelch(self._h, ch, float(level)))

    def set_ssb_squelch(self, enabled, level):
        check(self._L.qh_qps_set_ssb_squelch(self._h, 1 if enabled else 0, int(level)))

    def set_pieces(self, pieces):
        check(self._L.qh_qps_set_pieces(self._h, int(pieces)))

    def set_pipelined(self, on):
        """a call returns with its AGC still running; outputs are complete after synchronize()"""
        check(self._L.qh_qps_set_pipelined(self._h, 1 if on else 0))

    def out_capacity(self, n_in):
        return self._L.qh_qps_out_capacity(self._h, n_in)

    def process_ptr(self, d_in, in_stride, n, d_out, out_stride):
        got = C.c_int(0)
        check(self._L.qh_qps_process(self._h, d_in, in_stride, n, d_out, out_stride, C.byref(got)))
        return got.value

    def process_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise ValueError("expected [nch, n] complex128")
        cap = max(self.out_capacity(x.shape[1]), 1)
        out = np.empty((self.nch, cap), dtype=np.complex128)
        got = C.c_int(0)
        check(self._L.qh_qps_process_host(self._h, x.ctypes.data, x.shape[1], x.shape[1], out.ctypes.data, cap, C.byref(got)))
        return out[:, :got.value].copy()

    def squelch_flags(self):
        f = np.zeros(self.nch, dtype=np.int32)
        check(self._L.qh_qps_squelch_flags(self._h, f.ctypes.data))
        return f

    def get_graph(self, zoom=1.0, deltaf=0.0):
        pix = np.empty((self.nch, self.data_width), dtype=np.float64)
        sm = np.empty(self.nch, dtype=np.float64)
        cnt = C.c_int(0)
        check(self._L.qh_qps_get_graph(self._h, float(zoom), float(deltaf), pix.ctypes.data, sm.ctypes.data, C.byref(cnt)))
        return None if cnt.value <= 0 else (pix, sm, cnt.value)

    def synchronize(self):
        check(self._L.qh_qps_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_qps_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuiskAgc:
    """process_agc (quisk.c:2162-2287) for `nch` streams; the first process call only initialises, as in the reference."""

    def __init__(self, nch, sample_rate=48000, max_out=0.7, release_time=1.0, is_cpx=False, device=0, stream=None):
        self._L = load()
        self._h = self._L.qh_qagc_create(device, nch, sample_rate, max_out, release_time, 1 if is_cpx else 0, stream)
        if not self._h:
            raise QuiskHipError("qh_qagc_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch = nch

    def set_agc(self, ch, release_gain):
        check(self._L.qh_qagc_set_gain(self._h, ch, float(release_gain)))

    def process_ptr(self, d_buf, stride, n):
        check(self._L.qh_qagc_process(self._h, d_buf, stride, n))

    def process2_ptr(self, d_src, src_stride, d_dst, dst_stride, n):
        """from one device buffer into another"""
        check(self._L.qh_qagc_process2(self._h, d_src, src_stride, d_dst, dst_stride, n))

    def debug_form(self, form):
        """diagnostics: 0 = the two regimes as instruction chains (default), 1 = the whole machine sample by sample (bit-identical)"""
        check(self._L.qh_qagc_debug_form(self._h, int(form)))

    def process_host(self, x):
        buf = np.ascontiguousarray(x, dtype=np.complex128).copy()
        if buf.ndim != 2 or buf.shape[0] != self.nch:
            raise ValueError("expected [nch, n] complex128")
        check(self._L.qh_qagc_process_host(self._h, buf.ctypes.data, buf.shape[1], buf.shape[1]))
        return buf

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_qagc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NoiseBlanker:
    """NoiseBlanker (quisk.c:680-784) for `nch` streams at the receiver's input rate; level 0..3 as set_noise_blanker."""

    def __init__(self, nch, sample_rate, level=1, device=0, stream=None):
        self._L = load()
        self._h = self._L.qh_nb_create(device, nch, sample_rate, stream)
        if not self._h:
            raise QuiskHipError("qh_nb_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch = nch
        self.delay = self._L.qh_nb_delay(self._h)
        self.set_level(level)

    def set_level(self, level):
        check(self._L.qh_nb_set_level(self._h, int(level)))

    def reset(self):
        check(self._L.qh_nb_reset(self._h))

    def process_ptr(self, d_in, in_stride, d_out, out_stride, n):
        """Device pointers, strides in complex samples; d_in != d_out.  Asynchronous on the blanker's stream."""
        check(self._L.qh_nb_process(self._h, d_in, in_stride, d_out, out_stride, n))

    def process_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise ValueError("expected [nch, n] complex128")
        out = np.empty_like(x)
        check(self._L.qh_nb_process_host(self._h, x.ctypes.data, x.shape[1], out.ctypes.data, x.shape[1], x.shape[1]))
        return out

    def synchronize(self):
        check(self._L.qh_nb_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_nb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _WdspBlankerBank:
    """What WdspNoiseBlanker and WdspNoiseBlanker2 share: a bank handle of the C names `_prefix` + ..., its setters and its calls."""

    _prefix = None

    def _open(self, nch, *args):
        self._L = load()
        self._h = self._c("create")(*args)
        if not self._h:
            raise QuiskHipError("%screate failed: %s" % (self._prefix, self._L.qh_last_error().decode(errors="replace")))
        self.nch = nch

    def _c(self, name):
        return getattr(self._L, self._prefix + name)

    def set_run(self, run, ch=-1):
        check(self._c("set_run")(self._h, ch, int(run)))

    def set_samplerate(self, samplerate, ch=-1):
        check(self._c("set_samplerate")(self._h, ch, samplerate))

    def set_tau(self, tau, ch=-1):
        check(self._c("set_tau")(self._h, ch, tau))

    def set_hangtime(self, hangtime, ch=-1):
        check(self._c("set_hangtime")(self._h, ch, hangtime))

    def set_advtime(self, advtime, ch=-1):
        check(self._c("set_advtime")(self._h, ch, advtime))

    def set_backtau(self, backtau, ch=-1):
        check(self._c("set_backtau")(self._h, ch, backtau))

    def set_threshold(self, threshold, ch=-1):
        check(self._c("set_threshold")(self._h, ch, threshold))

    def flush(self, ch=-1):
        check(self._c("flush")(self._h, ch))

    def process_ptr(self, d_in, in_stride, d_out, out_stride, n):
        """Device pointers, strides in complex samples; rows of d_out apart from those of d_in.  Asynchronous on the bank's stream."""
        check(self._c("process")(self._h, d_in, in_stride, d_out, out_stride, n))

    def process_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise ValueError("expected [nch, n] complex128")
        out = np.empty_like(x)
        check(self._c("process_host")(self._h, x.ctypes.data, x.shape[1], out.ctypes.data, x.shape[1], x.shape[1]))
        return out

    def synchronize(self):
        check(self._c("synchronize")(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WdspNoiseBlanker(_WdspBlankerBank):
    """WDSP's noise blanker ANB (xanb, wdsp/nob.c:107-187) for `nch` streams at the receiver's input rate, every channel with its own
    settings; keyword names as create_anb's.  The setters take a channel, or -1 for every channel."""

    _prefix = "qh_anb_"

    def __init__(self, nch, samplerate, tau=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0, device=0, stream=None):
        self._open(nch, device, nch, samplerate, tau, hangtime, advtime, backtau, threshold, stream)

    def delay(self, ch=0):
        """trans_count + adv_count of channel ch: how far its output lags its input while it runs."""
        return self._c("delay")(self._h, ch)


class WdspNoiseBlanker2(_WdspBlankerBank):
    """WDSP's second noise blanker NOB, the callers' "NB2" (xnob, wdsp/nobII.c:157-495) for `nch` streams at the receiver's input rate,
    every channel with its own settings; keyword names as create_nobEXT's.  mode: 0 zeros, 1 hold the clean samples before the blank, 2
    the mean of before and after, 3 after, 4 a line between them.  The setters take a channel, or -1 for every channel."""

    _prefix = "qh_nob_"

    def __init__(self, nch, samplerate, mode=0, slewtime=1e-4, hangtime=1e-4, advtime=1e-4, backtau=0.05, threshold=30.0, device=0, stream=None):
        self._open(nch, device, nch, samplerate, int(mode), slewtime, hangtime, advtime, backtau, threshold, stream)

    def delay(self, ch=0):
        """How far the output of channel ch lags its input while it runs (adv_slew + adv + 1 + max_imp_seq + hang + hang_slew + 10)."""
        return self._c("delay")(self._h, ch)

    def set_mode(self, mode, ch=-1):
        check(self._c("set_mode")(self._h, ch, int(mode)))


class WdspVarResampler:
    """WDSP's variable-ratio resampler VARSAMP (xvarsamp, wdsp/varsamp.c:124-179) for `nch` streams, every channel with its own design,
    varmode, run and state; keyword names as create_varsamp's.  A call takes n input samples and one ratio correction `var` per channel
    and makes about n * var * out_rate / in_rate samples of every channel: the counts come back with the samples.  The setters take a
    channel, or -1 for every channel."""

    def __init__(self, nch, in_rate, out_rate, R=1024, fc=0.0, fc_low=-1.0, gain=1.0, var=1.0, varmode=1, device=0, stream=None):
        self._L = load()
        self._h = self._L.qh_varsamp_create(device, nch, int(in_rate), int(out_rate), int(R), fc, fc_low, gain, var, int(varmode), stream)
        if not self._h:
            raise QuiskHipError("qh_varsamp_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch = nch

    def _var(self, var):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(var, dtype=np.float64), (self.nch,)))
        return v

    def set_run(self, run, ch=-1):
        check(self._L.qh_varsamp_set_run(self._h, ch, int(run)))

    def set_varmode(self, varmode, ch=-1):
        check(self._L.qh_varsamp_set_varmode(self._h, ch, int(varmode)))

    def set_rates(self, in_rate, out_rate, ch=-1):
        """setInRate_varsamp / setOutRate_varsamp: a new design, and the channel starts over"""
        check(self._L.qh_varsamp_set_rates(self._h, ch, int(in_rate), int(out_rate)))

    def set_bandwidth(self, fc_low, fc_high, ch=-1):
        check(self._L.qh_varsamp_set_bandwidth(self._h, ch, fc_low, fc_high))

    def flush(self, ch=-1):
        check(self._L.qh_varsamp_flush(self._h, ch))

    def rsize(self, ch=0):
        """the taps of one output sample of channel ch"""
        return self._L.qh_varsamp_rsize(self._h, ch)

    def max_out(self, n, var):
        """the largest count the next call of n samples with these var could report on any channel"""
        v = self._var(var)
        m = self._L.qh_varsamp_max_out(self._h, int(n), v.ctypes.data)
        if m < 0:
            check(int(m))
        return int(m)

    def process_ptr(self, d_in, in_stride, d_out, out_stride, n, var, d_count=None):
        """Device pointers, strides in complex samples, out_stride >= max_out(n, var); rows of d_out apart from those of d_in; d_count:
        device int[nch] or None.  Asynchronous on the bank's stream."""
        v = self._var(var)
        check(self._L.qh_varsamp_process(self._h, d_in, in_stride, d_out, out_stride, n, v.ctypes.data, d_count))

    def process_host(self, x, var):
        """x [nch, n] complex128, var a number or [nch] -> (y [nch, max_out], counts [nch]); row c of y holds counts[c] samples, zeros behind"""
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise ValueError("expected [nch, n] complex128")
        v = self._var(var)
        n = x.shape[1]
        mo = max(self.max_out(n, v), 1)
        out = np.zeros((self.nch, mo), dtype=np.complex128)
        counts = np.zeros(self.nch, dtype=np.int32)
        check(self._L.qh_varsamp_process_host(self._h, x.ctypes.data, max(n, 1), out.ctypes.data, mo, n, v.ctypes.data, counts.ctypes.data))
        return out, counts

    def synchronize(self):
        check(self._L.qh_varsamp_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_varsamp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WdspResampler:
    """WDSP's fixed-ratio resampler (xresample / xresampleF, wdsp/resample.c:121-157, 296-330) for `nch` streams, every channel with its
    own design, run and state; keyword names as create_resample's.  dtype "c64": complex128 samples; "r32": float32 samples with the
    ring, the taps and the sums in doubles and create_resampleF's design (fc, ncoef and gain are not used there).  A call takes n input
    samples and makes ceil((n L - phnum) / M) of every channel: the counts come back with the samples.  The setters take a channel, or
    -1 for every channel."""

    C64, R32 = 0, 1

    def __init__(self, nch, in_rate, out_rate, fc=0.0, ncoef=0, gain=1.0, dtype="c64", device=0, stream=None):
        self._L = load()
        if dtype not in ("c64", "r32"):
            raise ValueError("dtype is 'c64' or 'r32'")
        self.dtype = dtype
        self.np_dtype = np.complex128 if dtype == "c64" else np.float32
        self._h = self._L.qh_resample_create(device, nch, int(in_rate), int(out_rate), fc, int(ncoef), gain, self.C64 if dtype == "c64" else self.R32,
                                             stream)
        if not self._h:
            raise QuiskHipError("qh_resample_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.nch = nch
        self._own_stream = stream is None

    def set_run(self, run, ch=-1):
        check(self._L.qh_resample_set_run(self._h, ch, int(run)))

    def set_rates(self, in_rate, out_rate, ch=-1):
        """setInRate_resample / setOutRate_resample: a new design, and the channel starts over"""
        check(self._L.qh_resample_set_rates(self._h, ch, int(in_rate), int(out_rate)))

    def set_fc_low(self, fc_low, ch=-1):
        check(self._L.qh_resample_set_fc_low(self._h, ch, fc_low))

    def set_bandwidth(self, fc_low, fc_high, ch=-1):
        check(self._L.qh_resample_set_bandwidth(self._h, ch, fc_low, fc_high))

    def flush(self, ch=-1):
        check(self._L.qh_resample_flush(self._h, ch))

    def L(self, ch=0):
        return self._L.qh_resample_L(self._h, ch)

    def M(self, ch=0):
        return self._L.qh_resample_M(self._h, ch)

    def cpp(self, ch=0):
        """the taps of one output sample of channel ch"""
        return self._L.qh_resample_cpp(self._h, ch)

    def taps(self, ch=0):
        """the phase-major h[L, cpp] in force on channel ch"""
        h = np.empty((self.L(ch), self.cpp(ch)), dtype=np.float64)
        r = self._L.qh_resample_taps(self._h, ch, h.ctypes.data, h.size)
        if r != h.size:
            check(r if r < 0 else -2)
        return h

    def out_count(self, n, ch=0):
        """what the next call of n samples makes of channel ch"""
        m = self._L.qh_resample_out_count(self._h, ch, int(n))
        if m < 0:
            check(int(m))
        return int(m)

    def max_out(self, n):
        """the most samples a call of n samples can write to any output row"""
        m = self._L.qh_resample_max_out(self._h, int(n))
        if m < 0:
            check(int(m))
        return int(m)

    def process_ptr(self, d_in, in_stride, d_out, out_stride, n):
        """Device pointers, strides in samples, out_stride >= max_out(n); rows of d_out apart from those of d_in.  Asynchronous on the
        bank's stream -> counts [nch]"""
        counts = np.zeros(self.nch, dtype=np.int32)
        check(self._L.qh_resample_process(self._h, d_in, in_stride, d_out, out_stride, int(n), counts.ctypes.data))
        return counts

    def process(self, x, out=None):
        """x: a torch device tensor [nch, n] of the bank's sample type, rows contiguous -> (y [nch, max_out(n)], counts [nch]); row c of y
        holds counts[c] samples.  `out`: a tensor to write to in place of a new one.  Asynchronous on the bank's stream: y is complete
        after synchronize().  A bank made with stream=None runs on a stream of its own, so torch's current stream is waited for first
        (x has to be there); pass stream=torch.cuda.current_stream().cuda_stream to stay in torch's order with no wait at all."""
        import torch
        want = torch.complex128 if self.dtype == "c64" else torch.float32
        if x.dim() != 2 or x.shape[0] != self.nch or x.dtype != want or not x.is_cuda or x.stride(1) != 1:
            raise ValueError("expected a device tensor [nch, n] of %s with contiguous rows" % want)
        n = x.shape[1]
        mo = max(self.max_out(n), 1)
        if out is None:
            out = torch.zeros((self.nch, mo), dtype=want, device=x.device)
        elif out.dim() != 2 or out.shape[0] != self.nch or out.dtype != want or not out.is_cuda or out.stride(1) != 1 or out.shape[1] < mo:
            raise ValueError("out: a device tensor [nch, >= max_out(n)] of %s with contiguous rows" % want)
        if self._own_stream:
            torch.cuda.current_stream(x.device).synchronize()
        return out, self.process_ptr(x.data_ptr(), x.stride(0) if n else 1, out.data_ptr(), out.stride(0), n)

    def process_host(self, x):
        """x [nch, n] -> (y [nch, max_out(n)], counts [nch]); row c of y holds counts[c] samples (the n copied ones of a channel that
        does not run), zeros behind"""
        x = np.ascontiguousarray(x, dtype=self.np_dtype)
        if x.ndim != 2 or x.shape[0] != self.nch:
            raise ValueError("expected [nch, n]")
        n = x.shape[1]
        mo = max(self.max_out(n), 1)
        out = np.zeros((self.nch, mo), dtype=self.np_dtype)
        counts = np.zeros(self.nch, dtype=np.int32)
        check(self._L.qh_resample_process_host(self._h, x.ctypes.data, max(n, 1), out.ctypes.data, mo, n, counts.ctypes.data))
        return out, counts

    def synchronize(self):
        check(self._L.qh_resample_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_resample_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WdspDiversity:
    """WDSP's diversity combiner DIV (xdiv, wdsp/div.c:67-95) for `ngroups` groups of up to eight phase-coherent receivers, every group
    with its own run, nr, output and rotate factors.  run = 0 gives receiver 0, output != nr gives receiver `output`, output == nr the sum
    of the receivers times their complex rotate factors, bit for bit the reference's.  The setters take a group, or -1 for every group."""

    MAX_NR = 8

    def __init__(self, ngroups, nr, run=1, device=0, stream=None):
        self._L = load()
        self._h = self._L.qh_div_create(device, ngroups, int(run), int(nr), stream)
        if not self._h:
            raise QuiskHipError("qh_div_create failed: %s" % self._L.qh_last_error().decode(errors="replace"))
        self.ngroups = ngroups

    def set_run(self, run, g=-1):
        check(self._L.qh_div_set_run(self._h, g, int(run)))

    def set_nr(self, nr, g=-1):
        check(self._L.qh_div_set_nr(self._h, g, int(nr)))

    def set_output(self, output, g=-1):
        """which receiver to put out; output == nr mixes"""
        check(self._L.qh_div_set_output(self._h, g, int(output)))

    def set_rotate(self, irotate, qrotate, g=-1):
        """the rotate factors of the first len(irotate) receivers (SetEXTDIVRotate's nr is the length)"""
        ir = np.ascontiguousarray(irotate, dtype=np.float64).ravel()
        qr = np.ascontiguousarray(qrotate, dtype=np.float64).ravel()
        if ir.size != qr.size:
            raise ValueError("irotate and qrotate differ in length")
        check(self._L.qh_div_set_rotate(self._h, g, int(ir.size), ir.ctypes.data, qr.ctypes.data))

    def get(self, g):
        """-> dict(run, nr, output, irotate[8], qrotate[8]) as the next call will use them"""
        run, nr, output = C.c_int(0), C.c_int(0), C.c_int(0)
        ir, qr = np.zeros(self.MAX_NR), np.zeros(self.MAX_NR)
        check(self._L.qh_div_get(self._h, g, C.byref(run), C.byref(nr), C.byref(output), ir.ctypes.data, qr.ctypes.data))
        return dict(run=run.value, nr=nr.value, output=output.value, irotate=ir, qrotate=qr)

    def process_ptr(self, d_in, rx_stride, group_stride, d_out, out_stride, n):
        """Device pointers, strides in complex samples: receiver i of group g at d_in + g group_stride + i rx_stride, its output at d_out +
        g out_stride.  d_out may be d_in + k rx_stride with out_stride == group_stride (the reference's out == in[k]); any other overlap
        is refused.  Asynchronous on the bank's stream."""
        check(self._L.qh_div_process(self._h, d_in, rx_stride, group_stride, d_out, out_stride, n))

    def process_host(self, x, onto=None):
        """x [ngroups, nr_max, n] complex128 -> [ngroups, n].  onto=k lays the output over receiver k as the reference's callers do with
        out == in[k]: the result is what the reference leaves there (x itself is not changed)."""
        x = np.ascontiguousarray(x, dtype=np.complex128)
        if x.ndim != 3 or x.shape[0] != self.ngroups:
            raise ValueError("expected [ngroups, nr_max, n] complex128")
        nrm, n = x.shape[1], x.shape[2]
        if onto is None:
            out = np.empty((self.ngroups, n), dtype=np.complex128)
            check(self._L.qh_div_process_host(self._h, x.ctypes.data, max(n, 1), max(nrm * n, 1), out.ctypes.data, max(n, 1), n))
            return out
        k = int(onto)
        if not 0 <= k < nrm:
            raise ValueError("onto must name one of the receivers of x")
        buf = x.copy()
        check(self._L.qh_div_process_host(self._h, buf.ctypes.data, max(n, 1), max(nrm * n, 1), buf[:, k].ctypes.data, max(nrm * n, 1), n))
        return buf[:, k].copy()

    def synchronize(self):
        check(self._L.qh_div_synchronize(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.qh_div_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
