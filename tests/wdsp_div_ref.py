"""A literal restatement of WDSP's diversity combiner (wdsp/div.c: create_div :31-48, xdiv :67-95, the setters :136-187) in numpy, for
the tests of qh_div_* and the EXT names.

xdiv(ins, out) works on the arrays it is handed -- complex128 rows, whose .real / .imag are views of the interleaved doubles -- so passing
the same array as `out` and as ins[k] aliases as it does in C: the memset zeroes that receiver's samples and the loop reads the running
sum back at i = k.  The loop over the receivers is outside, as in the reference, and the samples are vectorised inside: no sample looks
at another one.  Every product, the difference and the sum inside the bracket and the accumulation are separate float64 operations (numpy
fuses nothing), as the reference's statements are when its compiler does not contract them."""
import numpy as np

MAX_NR = 8                                              # div.c:29


def _same(a, b):
    """a->out != a->in[a->output], div.c:74: the pointers"""
    return a.__array_interface__["data"][0] == b.__array_interface__["data"][0]


class Div:
    def __init__(self, run, nr):                        # create_div, div.c:31-48 (malloc0: output 0, rotates 0)
        self.run = run
        self.nr = nr
        self.output = 0
        self.Irotate = np.zeros(MAX_NR)
        self.Qrotate = np.zeros(MAX_NR)

    def SetRun(self, run):                              # div.c:137-144
        self.run = run

    def SetNr(self, nr):                                # div.c:157-164
        self.nr = nr

    def SetOutput(self, output):                        # div.c:168-175
        self.output = output

    def SetRotate(self, nr, Irotate, Qrotate):          # div.c:179-187: this nr is the call's own
        self.Irotate[:nr] = np.asarray(Irotate, dtype=np.float64)[:nr]
        self.Qrotate[:nr] = np.asarray(Qrotate, dtype=np.float64)[:nr]

    def xdiv(self, ins, out):
        """ins: a list of at least nr complex128 rows, out: a complex128 row of the same length (may be one of ins); returns out"""
        if self.run:
            if self.output != self.nr:
                if not _same(out, ins[self.output]):
                    out[:] = ins[self.output]                                   # div.c:75
            else:
                out[:] = 0.0                                                    # div.c:81
                for i in range(self.nr):
                    I = ins[i].real.copy()                                      # div.c:85-86 (read before out[2j] moves)
                    Q = ins[i].imag.copy()
                    a = self.Irotate[i] * I
                    b = self.Qrotate[i] * Q
                    c = self.Irotate[i] * Q
                    d = self.Qrotate[i] * I
                    re = a - b
                    im = c + d
                    out.real[:] = out.real + re                                 # div.c:87
                    out.imag[:] = out.imag + im                                 # div.c:88
        else:
            out[:] = ins[0]                                                     # div.c:94
        return out


def mix(run, nr, output, Irotate, Qrotate, rows, onto=None):
    """One xdiv on copies of `rows` ([>= nr, n] complex128) with these settings; onto=k hands out == in[k].  Returns the output row."""
    d = Div(run, nr)
    d.SetOutput(output)
    d.SetRotate(len(Irotate), Irotate, Qrotate)
    ins = [np.array(r, dtype=np.complex128) for r in rows]
    out = ins[onto] if onto is not None else np.full(ins[0].shape, np.nan + 1j * np.nan)
    return d.xdiv(ins, out)
