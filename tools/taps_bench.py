"""What the RXA engine's sender and siphon taps cost at one GPU's share of BASELINE config 2 (256 channels, USB, 2^20 dsp samples per
channel and call, fp64: bench.py's settings), where a taps-off call takes the linear path and a call with a tap the per-mode path.  One
process, four cases in turn on one engine: taps off, the sender on in every channel, the siphon on in every channel, both on with a bank
of 256 displays attached.  Per case the engine's own event timing (qh_rxa_enable_timing: front / band / rest, ms) of one call and the wall
time per call of `steps` calls, the display's work included where one is attached.  One JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import quisk_amd as qh
    from quisk_amd import synth
    nch, nblk = int(os.environ.get("QH_TAPS_NCH", "256")), int(os.environ.get("QH_TAPS_NBLK", "4096"))
    steps = int(os.environ.get("QH_TAPS_STEPS", "3"))
    dev = torch.device("cuda:0")
    n_in, n_out = nblk * 1024, nblk * 256
    e = qh.RxaEngine(nch)
    e.SetRXAShiftRun(-1, 1)
    for c in range(nch):
        e.SetRXAShiftFreq(c, synth.shift_freq(c))
    e.RXANBPSetRun(-1, 1); e.SetRXAMode(-1, 1); e.RXASetPassband(-1, 300.0, 3000.0)
    e.SetRXAAGCMode(-1, 0); e.SetRXAAGCFixed(-1, 0.0)
    x = synth.make_input_torch(nch, n_in, dev, fs=192000.0)
    y = torch.empty((nch, n_out), dtype=torch.complex128, device=dev)
    bank = qh.AnalyzerBank(nch, 1024)
    bank.SetDisplaySampleRate(48000)
    bank.SetAnalyzer(1, 1, 1, [0], 1024, 256, 2, 0.0, 512, 0, 0.0, 0.0, 400, 1, 0, 0.0, 0.0, 2048)

    def sync():
        e.synchronize()
        torch.cuda.synchronize(dev)

    def case(name):
        step = lambda: e.process_ptr(x.data_ptr(), n_in, y.data_ptr(), n_out, nblk)
        for _ in range(2):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        wall = (time.perf_counter() - t0) / steps * 1e3
        e.enable_timing(True)
        step()
        ev = e.timing_ms()
        e.enable_timing(False)
        sync()
        return {"case": name, "wall_ms_per_call": round(wall, 3), "event_ms": [round(v, 3) for v in ev], "event_ms_sum": round(sum(ev), 3),
                "device_bytes": e.device_bytes()}

    out = [case("taps off")]
    e.set_sender(-1, 1)
    out.append(case("sender on"))
    e.set_sender(-1, 0); e.set_siphon(-1, 1)
    out.append(case("siphon on"))
    e.attach_display(bank, 0)
    frames = bank.frames()
    out.append(case("sender + siphon on, %d displays attached" % nch))
    out[-1]["display_frames_per_call"] = (bank.frames() - frames) // (steps + 3)
    e.attach_display(None)
    print(json.dumps({"config": "2 (one GPU's share): %d ch x 192 k, %d blocks a call" % (nch, nblk), "cases": out}))
    e.close(); bank.close()


if __name__ == "__main__":
    main()
