"""The AGC's display-side knobs (wdsp/wcpAGC.c:440-557) written out in Python on the values loadWcpAGC derives (wcpAGC.c:115-146), with
create_rxa's constants (RXA.c:335-358: out_targ 1.0, n_tau 4, max_gain 10000, var_gain 1.5, max_input 1.0, hang_thresh 0.25), and
oracle/wcpagc_oracle's wo_agc as a ctypes structure, so that a test can run the restated xwcpagc on samples of its own with any of its
public fields set.  numpy and the oracle library only."""
import ctypes as C
import math

import numpy as np

OUT_TARG, N_TAU = 1.0, 4                                # RXA.c:350,345
MAX_GAIN, VAR_GAIN, MAX_INPUT, HANG_THRESH = 10000.0, 1.5, 1.0, 0.250      # RXA.c:346-347,349,357
NBP_BAND = (-4150.0, -150.0)                            # nbp0's edges as create_rxa leaves them (RXA.c:99-100)


def out_target():
    return OUT_TARG * (1.0 - math.exp(-float(N_TAU))) * 0.9999


def min_volts(max_gain=MAX_GAIN, var_gain=VAR_GAIN):
    return out_target() / (var_gain * max_gain)


def noise_offset(band, size, rate):
    return 10.0 * math.log10((band[1] - band[0]) * size / rate)


def thresh_to_max_gain(thresh, size, rate, band=NBP_BAND, var_gain=VAR_GAIN):
    """SetRXAAGCThresh, wcpAGC.c:499-511"""
    return out_target() / (var_gain * 10.0 ** ((thresh + noise_offset(band, size, rate)) / 20.0))


def max_gain_to_thresh(max_gain, size, rate, band=NBP_BAND, var_gain=VAR_GAIN):
    """GetRXAAGCThresh, wcpAGC.c:487-497"""
    return 20.0 * math.log10(min_volts(max_gain, var_gain)) - noise_offset(band, size, rate)


def hang_level_to_thresh(level, max_gain=MAX_GAIN, var_gain=VAR_GAIN, max_input=MAX_INPUT):
    """SetRXAAGCHangLevel, wcpAGC.c:449-466: hang_thresh"""
    mv = min_volts(max_gain, var_gain)
    if max_input > mv:
        convert = 10.0 ** (level / 20.0)
        tmp = max(1e-8, (convert - mv) / (max_input - mv))
        return 1.0 + 0.125 * math.log10(tmp)
    return 1.0


def hang_level(hang_thresh, max_gain=MAX_GAIN, var_gain=VAR_GAIN, max_input=MAX_INPUT):
    """loadWcpAGC's hang_level, wcpAGC.c:139-141"""
    tmp = 10.0 ** ((hang_thresh - 1.0) / 0.125)
    return (max_input * tmp + (out_target() / (var_gain * max_gain)) * (1.0 - tmp)) * 0.637


def thresh_to_hang_level(hang_thresh, max_gain=MAX_GAIN, var_gain=VAR_GAIN, max_input=MAX_INPUT):
    """GetRXAAGCHangLevel, wcpAGC.c:440-447"""
    return 20.0 * math.log10(hang_level(hang_thresh, max_gain, var_gain, max_input) / 0.637)


def solve_hang_level(hang_thresh, max_gain=MAX_GAIN, var_gain=VAR_GAIN, max_input=MAX_INPUT):
    """The level (dB) whose SetRXAAGCHangLevel gives hang_thresh: the inverse of hang_level_to_thresh on its first branch"""
    mv = min_volts(max_gain, var_gain)
    assert max_input > mv
    tmp = 10.0 ** ((hang_thresh - 1.0) / 0.125)
    return 20.0 * math.log10(tmp * (max_input - mv) + mv)


class WoAgc(C.Structure):
    """wo_agc, oracle/wcpagc_oracle.h:10-20"""
    _fields_ = ([(n, C.c_int) for n in ("run", "mode", "pmode", "n_tau", "hang_enable")] +
                [(n, C.c_double) for n in ("sample_rate", "tau_attack", "tau_decay", "max_gain", "var_gain", "fixed_gain", "max_input", "out_targ",
                                           "tau_fast_backaverage", "tau_fast_decay", "pop_ratio", "tau_hang_backmult", "hangtime", "hang_thresh",
                                           "tau_hang_decay")] +
                [(n, C.c_int) for n in ("ring_buffsize", "attack_buffsize", "in_index", "out_index", "hang_counter", "decay_type", "state")] +
                [(n, C.c_double) for n in ("attack_mult", "decay_mult", "fast_decay_mult", "fast_backmult", "onemfast_backmult", "out_target",
                                           "min_volts", "inv_out_target", "slope_constant", "inv_max_input", "hang_level", "hang_backmult",
                                           "onemhang_backmult", "hang_decay_mult", "ring_max", "volts", "save_volts", "fast_backaverage",
                                           "hang_backaverage", "gain")] +
                [("ring", C.c_void_p), ("abs_ring", C.c_void_p)])


class RxaAgc:
    """The wcpAGC of an RXA channel as create_rxa makes it (RXA.c:335-358), mode 3; fields are set through `set` and loaded"""

    def __init__(self, oracle, rate=48000, mode=3):
        self.L = oracle.lib()
        self.L.wo_agc_init.argtypes = ([C.c_void_p] + [C.c_int] * 4 + [C.c_double] * 2 + [C.c_int] + [C.c_double] * 8 + [C.c_int] +
                                       [C.c_double] * 4)
        self.L.wo_agc_init.restype = None
        for n in ("wo_agc_free", "wo_agc_load"):
            getattr(self.L, n).argtypes = [C.c_void_p]
            getattr(self.L, n).restype = None
        self.L.wo_agc_set_mode.argtypes = [C.c_void_p, C.c_int]
        self.L.wo_agc_set_mode.restype = None
        self.L.wo_agc_exec.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.L.wo_agc_exec.restype = None
        self.a = WoAgc()
        self.L.wo_agc_init(C.byref(self.a), 1, 3, 1, rate, 0.001, 0.250, 4, 10000.0, 1.5, 1000.0, 1.0, 1.0, 0.250, 0.005, 5.0, 1, 0.500, 0.250, 0.250,
                           0.100)
        self.L.wo_agc_set_mode(C.byref(self.a), mode)

    def set(self, **fields):
        for k, v in fields.items():
            setattr(self.a, k, v)
        self.L.wo_agc_load(C.byref(self.a))

    def __call__(self, x, block=64):
        y = np.ascontiguousarray(x, dtype=np.complex128).copy()
        assert y.size % block == 0
        for b in range(0, y.size, block):
            self.L.wo_agc_exec(C.byref(self.a), y[b:].ctypes.data, block)
        return y

    def close(self):
        if self.a.ring:
            self.L.wo_agc_free(C.byref(self.a))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
