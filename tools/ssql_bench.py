"""Time of xssql (qh_ssql.hpp) at the bench's config-2 shape: 256 channels, 2^20 dsp samples per channel and call (4096 blocks of 1024
input samples at 192 k -> 48 k), fp64.  One JSON line: the whole call with SSQL off, with SSQL on every channel, the difference, and the
traffic floor.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python tools/ssql_bench.py` (ssql_*_kernel).

One pass over the rows moves 256 x 2^20 x 16 B = 4.29 GB; the detector reads them twice and the apply pass reads and writes them once
(17.2 GB, 2.1 ms at 8 TB/s); everything else is bits."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import quisk_amd as qh
    from quisk_amd import synth
    dev = torch.device("cuda:0")
    nch, nblk = int(os.environ.get("QH_SS_NCH", "256")), int(os.environ.get("QH_SS_NBLK", "4096"))
    steps, warmup = int(os.environ.get("QH_SS_STEPS", "5")), 2
    n_in, n_out = nblk * 1024, nblk * 256
    x = synth.make_mode_input_torch(["usb"] * nch, n_in, dev, periodic=True)
    y = torch.empty((nch, n_out), dtype=torch.complex128, device=dev)
    e = qh.RxaEngine(nch)
    for c in range(nch):
        e.SetRXAShiftRun(c, 1); e.SetRXAShiftFreq(c, synth.shift_freq(c)); e.RXANBPSetRun(c, 1); e.SetRXAMode(c, 1)
        e.RXASetPassband(c, 300.0, 3000.0); e.SetRXAAGCMode(c, 0); e.SetRXAAGCFixed(c, 0.0)
    torch.cuda.synchronize(dev)

    def timed():
        for _ in range(warmup):
            e.process_ptr(x.data_ptr(), n_in, y.data_ptr(), n_out, nblk)
        e.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(steps):
            e.synchronize()
            t0.record()
            e.process_ptr(x.data_ptr(), n_in, y.data_ptr(), n_out, nblk)
            e.synchronize()
            t1.record()
            torch.cuda.synchronize(dev)
            ms.append(t0.elapsed_time(t1))
        return sorted(ms)[len(ms) // 2]

    # (with SSQL on the engine leaves the linear path for the per-mode one: the fixed gain ahead of the squelch, the panel in an
    # output pass behind it -- the difference below includes that; the kernel trace separates the squelch's own kernels)
    off = timed()
    e.SetRXASSQLRun(-1, 1)
    on = timed()
    bytes_pass = nch * n_out * 16
    print(json.dumps({"nch": nch, "n_dsp": n_out, "ms_ssql_off": off, "ms_ssql_all": on, "ms_added": on - off,
                      "one_pass_GB": bytes_pass / 1e9, "floor_ms_3r1w_at_8TBps": 4 * bytes_pass / 8e12 * 1e3}))
    e.close()


if __name__ == "__main__":
    main()
