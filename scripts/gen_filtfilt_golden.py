"""Writes tests/golden/filtfilt_scipy.npz: scipy.signal.lfilter_zi / sosfilt_zi of the designs of gen_iir_golden.py (and
its butter8 sos), and scipy.signal.filtfilt / sosfiltfilt (method="pad") in float64 / complex128 on rows of 96 samples,
real and complex, for every padtype, with the default padlen and one explicit value -- data only.  The tests read the
file and need no scipy.  Run from the repository root:  python scripts/gen_filtfilt_golden.py
"""
import os

import numpy as np
from scipy import signal

from gen_iir_golden import N, ROOT, designs

PADTYPES = ("odd", "even", "constant", None)
PADLEN = 11                                               # the explicit value


def main():
    rs = np.random.RandomState(23)
    out = {}
    xr = rs.randn(1, N)                                   # one row each: 144 recorded outputs
    xc = rs.randn(1, N) + 1j * rs.randn(1, N)
    out["x_real"], out["x_cplx"] = xr, xc
    out["padlen"] = np.array(PADLEN)

    def record(name, run):
        for kind, x in (("real", xr), ("cplx", xc)):
            for padtype in PADTYPES:
                for tag, padlen in (("default", None), ("padlen", PADLEN)):
                    out[f"{name}_{kind}_{padtype or 'none'}_{tag}"] = run(x, padtype, padlen)

    for name, (b, a) in designs():
        out[f"{name}_b"], out[f"{name}_a"] = np.asarray(b), np.asarray(a)
        out[f"{name}_zi"] = signal.lfilter_zi(b, a)
        record(name, lambda x, padtype, padlen: signal.filtfilt(b, a, x, axis=-1, padtype=padtype, padlen=padlen))
    sos = signal.butter(8, 0.3, output="sos")
    out["butter8sos_sos"], out["butter8sos_zi"] = sos, signal.sosfilt_zi(sos)     # [n_sections, 2]
    # scipy's default padlen of sosfiltfilt subtracts the count of zero b2 / a2 from the bracket: recorded, and passed
    # explicitly by the tests (cplx.sosfiltfilt does not read the values)
    ntaps = 2 * len(sos) + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    out["butter8sos_default_padlen"] = np.array(3 * ntaps)
    record("butter8sos", lambda x, padtype, padlen: signal.sosfiltfilt(sos, x, axis=-1, padtype=padtype, padlen=padlen))
    path = os.path.join(ROOT, "tests", "golden", "filtfilt_scipy.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
