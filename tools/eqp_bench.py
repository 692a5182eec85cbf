"""Time of xeqp at one GPU's share of BASELINE config 2 (256 channels, USB, 2^20 dsp samples per channel and call, fp64: bench.py's
settings) and of config 4 (tools/bench_configs.py: mode by c mod 3 = USB / AM / FM).  One JSON line per configuration: the whole call with
the equalizer off, with it on in every channel (a ten-band profile), the difference, and the engine's own front / band / rest split of the
on-case (qh_rxa_enable_timing).  For the kernels' own times and counts run it under `rocprofv3 --kernel-trace --stats -- python
tools/eqp_bench.py` (QH_EQ_ONLY=off / on times one case alone, so that the off-case's kernel list can be set beside the parent commit's:
it must hold nothing new; QH_EQ_CONFIG=2 / 4 runs one configuration).  On a commit without the equalizer only the off-case runs."""
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

G10 = [0, -12, -12, -12, -1, 1, 4, 9, 12, -10, -10]        # the profile create_rxa keeps in a comment (RXA.c:260)


def setup_config2(torch, qh, dev, bc, nch=256, nblk=4096):
    from quisk_amd import synth
    n_in = nblk * 1024
    L = SimpleNamespace(nch=nch, nblk=nblk, n_in=n_in, n_out=nblk * 256)
    L.stream = bc.new_stream(torch, dev)
    L.eng = eng = qh.RxaEngine(nch, device=dev.index or 0, stream=L.stream.cuda_stream)
    eng.SetRXAShiftRun(-1, 1)
    for c in range(nch):
        eng.SetRXAShiftFreq(c, synth.shift_freq(c))
    eng.RXANBPSetRun(-1, 1); eng.SetRXAMode(-1, 1); eng.RXASetPassband(-1, 300.0, 3000.0)
    eng.SetRXAAGCMode(-1, 0); eng.SetRXAAGCFixed(-1, 0.0)
    L.x = synth.make_input_torch(nch, n_in, dev, fs=192000.0)
    L.y = torch.empty((nch, L.n_out), dtype=torch.complex128, device=dev)
    L.step = lambda: eng.process_ptr(L.x.data_ptr(), n_in, L.y.data_ptr(), L.n_out, nblk)
    torch.cuda.synchronize(dev)
    return L


def one(torch, qh, dev, bc, config, only, steps):
    L = setup_config2(torch, qh, dev, bc) if config == 2 else bc.setup_config4(torch, qh, dev)
    sync = lambda: torch.cuda.synchronize(dev)
    r = {"config": "%d (one GPU's share): %d ch x 192 k, %d blocks a call" % (config, L.nch, L.nblk)}
    has = hasattr(L.eng, "debug_eqp")
    if only != "on":
        r["ms_eq_off"] = bc.timed(L.step, sync, steps=steps, warmup=2) * 1e3
        r["device_bytes_off"] = L.eng.device_bytes()
    if only != "off" and has:
        L.eng.SetRXAGrphEQ10(-1, G10)
        L.eng.SetRXAEQRun(-1, 1)
        r["ms_eq_on"] = bc.timed(L.step, sync, steps=steps, warmup=2) * 1e3
        r["device_bytes_on"] = L.eng.device_bytes()
        L.eng.enable_timing(True)
        L.step()
        kt = L.eng.timing_ms()
        L.eng.enable_timing(False)
        r.update(front_ms_on=kt[0], band_ms_on=kt[1], rest_ms_on=kt[2])
        if "ms_eq_off" in r:
            r["ms_added"] = r["ms_eq_on"] - r["ms_eq_off"]
            r["ns_added_per_sample"] = r["ms_added"] * 1e6 / (L.nch * L.n_out)
    print(json.dumps(r), flush=True)
    L.eng.close()
    del L
    torch.cuda.empty_cache()


def main():
    import torch
    import quisk_amd as qh
    import bench_configs as bc
    dev = torch.device("cuda:0")
    only = os.environ.get("QH_EQ_ONLY", "")
    steps = int(os.environ.get("QH_EQ_STEPS", "5"))
    which = os.environ.get("QH_EQ_CONFIG", "")
    for config in (2, 4):
        if which in ("", str(config)):
            one(torch, qh, dev, bc, config, only, steps)


if __name__ == "__main__":
    main()
