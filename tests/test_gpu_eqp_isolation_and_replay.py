"""The equalizer beside other channels and under launch-sequence replay.  -m gpu.

An engine whose equalizers never run allocates and computes what it did before the stage existed.  A channel that turns its equalizer on
moves no other channel by a bit where no store straight to the caller's rows is in play; where one is (the (USB, AM, FM, FM) engine), a
call with an equalizer takes the output pass for every channel, and the others get the bits of that form -- the form QH_DBG_FORMS=2
selects without an equalizer -- whose distance from the store form is measured and printed here (DESIGN.md section 7 records it)."""
import numpy as np
import pytest

from test_gpu_rxa_eqp import AM, FM, G10, G4, P3, USB, _engine, _input

pytestmark = pytest.mark.gpu
MIXED = [USB, AM, FM, FM]


def _walk(e, x, calls, between=None):
    ys, pos = [], 0
    for k, nb in enumerate(calls):
        if between:
            between(k, e)
        ys.append(e.process_host(np.ascontiguousarray(x[:, pos:pos + nb * e.dsp_insize])))
        pos += nb * e.dsp_insize
    return np.concatenate(ys, 1)


@pytest.mark.parametrize("modes", [MIXED, [USB] * 4], ids=["mixed", "linear"])
def test_setters_without_run_leave_the_engine_as_it_was(qh, modes):
    """every equalizer setter but Run 1, and Run 0, on one engine, none on the other: the same bits, the same device bytes, no stage"""
    a, b = _engine(qh, modes), _engine(qh, modes)
    a.SetRXAGrphEQ(0, G4); a.SetRXAGrphEQ10(1, G10); a.SetRXAEQProfile(2, *P3); a.SetRXAEQNC(3, 4096); a.SetRXAEQNC(2, 1024)
    a.SetRXAEQMP(1, 1); a.SetRXAEQCtfmode(-1, 1); a.SetRXAEQWintype(-1, 1); a.SetRXAEQRun(-1, 0)
    x = _input(modes, 10 * 4096, 192000.0, True)
    try:
        for k in range(10):
            xa = np.ascontiguousarray(x[:, k * 4096:(k + 1) * 4096])
            assert np.array_equal(a.process_host(xa), b.process_host(xa)), k
        assert a.device_bytes() == b.device_bytes()
        assert a.debug_eqp(0) is None and a.debug_eqp(3) is None
    finally:
        a.close(); b.close()


def test_turning_it_on_moves_no_other_channel(qh):
    """(USB, USB with AGC mode 3, AM, FM): the AGC's state machine keeps every channel on the output pass, so no direct-store form is in
    play; channel 0 turns its equalizer on before the third call"""
    modes = [USB, USB, AM, FM]
    calls = (8, 8, 8, 40, 8, 3)
    x = _input(modes, sum(calls) * 1024, 192000.0, True)
    outs = []
    for k in range(2):
        e = _engine(qh, modes)
        e.SetRXAAGCMode(1, 3)

        def between(i, e):
            if k and i == 2:
                e.SetRXAGrphEQ10(0, G10); e.SetRXAEQRun(0, 1)
        try:
            outs.append(_walk(e, x, calls, between))
        finally:
            e.close()
    for c in (1, 2, 3):
        assert np.array_equal(outs[0][c], outs[1][c]), c
    first = sum(calls[:2]) * 256
    assert np.array_equal(outs[0][0, :first], outs[1][0, :first]) and not np.array_equal(outs[0][0, first:], outs[1][0, first:])


def test_in_the_direct_store_engine_the_others_get_the_output_pass_bits(qh, monkeypatch):
    """(USB, AM, FM, FM) with nothing behind the channels' last filters stores straight to the caller's rows; the equalizer sits behind
    those stores, so a call with one takes the output pass instead (as QH_DBG_FORMS=2 does).  The other channels: bit for bit that form's
    output, and so as far from the store form's as that form is without any equalizer -- measured here, printed, asserted as the bound."""
    calls = (8, 8, 40, 3)
    x = _input(MIXED, sum(calls) * 1024, 192000.0, True)

    def run(forms, eq):
        if forms:
            monkeypatch.setenv("QH_DBG_FORMS", str(forms))
        else:
            monkeypatch.delenv("QH_DBG_FORMS", raising=False)
        e = _engine(qh, MIXED)
        monkeypatch.delenv("QH_DBG_FORMS", raising=False)
        if eq:
            e.SetRXAGrphEQ10(0, G10); e.SetRXAEQRun(0, 1)
        try:
            return _walk(e, x, calls)
        finally:
            e.close()

    store, passed, eq = run(0, False), run(2, False), run(0, True)
    for c in (1, 2, 3):
        scale = np.abs(store[c]).max()
        form = np.abs(passed[c] - store[c]).max() / scale
        moved = np.abs(eq[c] - store[c]).max() / scale
        print("channel %d: output pass against store form %.3g of the peak, with channel 0's equalizer on %.3g" % (c, form, moved))
        assert np.array_equal(eq[c], passed[c]), c
        assert moved <= form
    assert not np.array_equal(eq[0], store[0])


def test_on_the_linear_path_the_others_take_the_pointwise_epilogue(qh):
    """All-USB, the equalizer the chain's last stage: the channels that do not run it get the output matrix from the pointwise pass behind
    nbp0 instead of from nbp0's store.  Both forms apply the same real 2x2 matrix to the same tile output, so they can differ by the
    roundings of a few multiplications and one addition per component: bounded here at 8 eps of the channel's peak, measured and printed
    (DESIGN.md section 7 records it)."""
    modes = [USB] * 4
    calls = (8, 8, 40, 3)
    x = _input(modes, sum(calls) * 1024, 192000.0, True)
    outs = []
    for k in range(2):
        e = _engine(qh, modes)
        if k:
            e.SetRXAGrphEQ10(0, G10); e.SetRXAEQRun(0, 1)
        try:
            outs.append(_walk(e, x, calls))
        finally:
            e.close()
    for c in (1, 2, 3):
        moved = np.abs(outs[1][c] - outs[0][c]).max() / np.abs(outs[0][c]).max()
        print("linear path, channel %d with channel 0's equalizer on: %.3g of the peak" % (c, moved))
        assert moved <= 8 * np.finfo(np.float64).eps, (c, moved)
    assert not np.array_equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("modes", [MIXED, [USB] * 4], ids=["mixed", "linear"])
def test_graph_replay_matches_the_plain_path(qh, modes):
    """replayed calls give the plain path's bits, call by call, over 40 calls: Run toggled, a profile change, a second channel joining and
    leaving the list"""
    import torch
    dev = torch.device("cuda:0")
    nch, nblk, ncall = 4, 12, 40
    x = _input(modes, ncall * nblk * 1024, 192000.0, True)
    res, launches = [], 0
    for replay in (False, True):
        e = _engine(qh, modes)
        e.SetRXAGrphEQ(0, G4); e.SetRXAEQRun(0, 1)
        e.set_graph_replay(replay)
        d_in = torch.zeros((nch, nblk * 1024), dtype=torch.complex128, device=dev)
        d_out = torch.zeros((nch, nblk * 256), dtype=torch.complex128, device=dev)
        ys = []
        try:
            for k in range(ncall):
                if k == 6:
                    e.SetRXAEQRun(0, 0)
                elif k == 11:
                    e.SetRXAEQRun(0, 1)
                elif k == 16:
                    e.SetRXAEQProfile(0, *P3)
                elif k == 22:
                    e.SetRXAGrphEQ10(3, G10); e.SetRXAEQRun(3, 1)
                elif k == 31:
                    e.SetRXAEQRun(3, 0)
                d_in.copy_(torch.from_numpy(np.ascontiguousarray(x[:, k * nblk * 1024:(k + 1) * nblk * 1024])))
                e.process_ptr(d_in.data_ptr(), nblk * 1024, d_out.data_ptr(), nblk * 256, nblk)
                torch.cuda.synchronize()
                ys.append(d_out.cpu().numpy())
            if replay:
                launches = e.graph_launches()
        finally:
            e.close()
        res.append(ys)
    assert launches > 0
    for k in range(ncall):
        assert np.array_equal(res[0][k], res[1][k]), k
