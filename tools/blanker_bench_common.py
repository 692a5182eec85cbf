"""The input and the timing loop tools/anb_bench.py and tools/nob_bench.py share."""
import time


def noise(torch, dev, nch, n):
    """[nch, n] complex128 Gaussian noise whose mean magnitude is the detectors' start value 1.0."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    x = torch.empty((nch, n), dtype=torch.complex128, device=dev)
    for c in range(nch):
        x[c] = torch.complex(torch.randn(n, dtype=torch.float64, device=dev, generator=gen), torch.randn(n, dtype=torch.float64, device=dev, generator=gen)) * 0.8
    return x


def add_pulses(torch, x, every):
    """One pulse of 2 samples, 60 times the noise, every `every` samples per channel, offset per channel; in place."""
    for c in range(x.shape[0]):
        p = torch.arange((37 * c) % every + 100, x.shape[1] - 2, every, device=x.device)
        x[c, p] += 48.0
        x[c, p + 1] += 48.0
    return x


def time_calls(bank, x, y, n, steps, warmup=2):
    """Milliseconds of each of `steps` calls, each waited for, after `warmup` calls."""
    for _ in range(warmup):
        bank.process_ptr(x.data_ptr(), n, y.data_ptr(), n, n)
    bank.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        bank.process_ptr(x.data_ptr(), n, y.data_ptr(), n, n)
        bank.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms
