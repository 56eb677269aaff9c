"""The planted peaks of tests/fftcc_peak_cases.py through the REFERENCE ITSELF (oracle/_ref/liboc_ref.so, the reference's FFTCC loops
compiled unmodified over the stand-in FFTW): it must write the closed-form integers, and its distance from ZNCC = 1 -- its float32
running sums of means and norms over the window -- is where the GPU bars of tests/test_gpu_fftcc_peaks.py come from
(fftcc_peak_cases.MEASURED, 4 x).  MEASURED is taken over every record of every queue (`python tests/fftcc_peak_cases.py --measure`,
a minute and a half); here every shape of every family runs again on a strided sample of its queue, sized by the stand-in DFT's work
per record (fftcc_peak_cases.reference_runs): the closed-form integers on each record, and a distance that may not exceed the
committed figure of its family.  Skipped where the reference tree is not mounted."""
import pytest

import fftcc_peak_cases as pc
from oracle import ref as oref

pytestmark = pytest.mark.skipif(not oref.available(), reason="reference tree not mounted: oracle/_ref cannot be built")


def _reference(ref, tar, radii, q):
    (oref.fftcc2d if len(radii) == 2 else oref.fftcc3d)(ref, tar, *radii, q)


CASES = [(2, f) for f in pc.FAMILIES2D] + [(3, f) for f in pc.FAMILIES3D]


@pytest.mark.parametrize("nd,family", CASES, ids=["%dD_%s" % c for c in CASES])
def test_reference_writes_the_closed_form_and_stays_within_its_measured_distance(nd, family):
    dist = pc.reference_distance(nd, family, True, _reference)       # asserts the integers
    assert 0.0 < dist <= pc.MEASURED["%dD" % nd][family], (family, dist)
