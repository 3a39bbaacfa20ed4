"""The hand-built progressive scans of tests/jpeg_prog_cases.py through k_prog_scan / k_prog_finalize (gamut_amd/csrc/jpeg_prog.hpp): a wave per
scan segment, scans that follow each other through progress words, a lane per bit in DC refinement scans, ballot and rank search in AC
refinement blocks.  Coefficients and max_zag are compared bit for bit with the oracle, in poisoned buffers with a guarded tail; a file the
reference refuses (or has no defined result for) has to come back refused, its neighbours intact.  tests/test_jpeg_prog_cases_cpu.py proves on
the CPU that every case stands on what its name says."""
import os

import numpy as np
import pytest

import jpeg_prog_cases as S
import jpeg_prog_ref as R
import oracle_lib as O
from test_jpeg_gpu import _decode_batch_device, dev_upload, handoff, unstuff_site      # noqa: F401 (fixtures)
from test_jpeg_scan_cases_gpu import entropy_decode, judge, no_host_redo               # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

CASES = S.corpus()
IMAGES = [c for c in CASES if c.verdict == "image"]
G = S.geometry()


@pytest.fixture(scope="module")
def expected():
    """the oracle's reading of every case, made once: (coefficients, max_zag) or None"""
    out = {}
    for c in CASES:
        try:
            d = O.DecodedJpeg(c.data)
            out[c.name] = (d.coeffs, d.max_zag)
        except ValueError:
            out[c.name] = None
    assert all((out[c.name] is not None) == (c.verdict == "image") for c in CASES)
    return out


@pytest.fixture(scope="module")
def pixels():
    """the oracle's pixels of every image case, 4 and 1 components, made once"""
    return {(c.name, comps): O.decompress_jpeg(c.data, comps)[0] for c in IMAGES for comps in (4, 1)}


@pytest.fixture
def progressive():
    """-> a function that sets GAMUT_HIP_JPEG_PROGRESSIVE for the test: 'device' = every scan in k_prog_scan, 'host' = the host feeder"""
    old = os.environ.get("GAMUT_HIP_JPEG_PROGRESSIVE")

    def use(mode):
        os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"] = mode
    yield use
    if old is None:
        os.environ.pop("GAMUT_HIP_JPEG_PROGRESSIVE", None)
    else:
        os.environ["GAMUT_HIP_JPEG_PROGRESSIVE"] = old


def test_the_whole_corpus_in_one_call_on_the_device(hip, progressive, expected):
    """every case in one launch of k_prog_scan: hundreds of scan segments, refused and undefined files between good ones"""
    progressive("device")
    rc, hst, st, res = entropy_decode(hip, [c.data for c in CASES])
    judge(CASES, hst, st, res, expected, "device, one call")
    assert (rc != 0) == any(hst)


def test_each_image_case_in_a_call_of_its_own(hip, progressive, expected):
    """a launch per file: its scans alone on the chip, every scan right behind the one it stands on"""
    progressive("device")
    for c in IMAGES:
        rc, hst, st, res = entropy_decode(hip, [c.data])
        assert rc == 0, (c.name, hip.gamut_hip_last_error())
        judge([c], hst, st, res, expected, "device, alone")


def test_the_corpus_on_the_host_feeder(hip, progressive, expected):
    progressive("host")
    rc, hst, st, res = entropy_decode(hip, [c.data for c in CASES])
    judge(CASES, hst, st, res, expected, "host")


def host_by_design(c):
    """what k_prog_scan hands to the host feeder by design: a stream no plain decoder follows (a bit pattern no code word begins), and one that
    reads further behind a segment than the padding the host puts there"""
    try:
        d = R.decode(c.data, habits=True)
    except (R.Undefined, IndexError):
        return True
    return any(s.past_end > G["padding"] * 8 for s in d.scans)


def test_the_kernel_decodes_every_well_formed_case_itself(hip, progressive, no_host_redo, expected):
    """with the host feeder's second reading switched off and every scan on the GPU: every stream T.81 defines and the reference decodes comes out of
    k_prog_scan itself, in one batch and alone; so do the streams that rest on a habit of the reference the kernel shares (a run that leaves its band
    or finds no position without history, an EOB run dropped at RSTn, a set bit plane, ones from the padding); the others stay refused"""
    progressive("device")
    own = [c for c in IMAGES if c.wellformed]
    habit = [c for c in IMAGES if not c.wellformed]
    theirs = [c for c in habit if host_by_design(c)]
    shared = [c for c in habit if not host_by_design(c)]
    assert len(own) >= 80 and len(shared) >= 15, (len(own), len(shared), len(theirs))
    batch = own + shared + theirs
    rc, hst, st, res = entropy_decode(hip, [c.data for c in batch])
    for c, h in zip(batch, hst):
        assert (h == 0) == (c not in theirs), (c.name, h)
    judge(own + shared, hst, st, res, expected, "no second reading")
    for c in own:
        rc, hst, st, res = entropy_decode(hip, [c.data])
        assert rc == 0 and hst == [0], (c.name, hip.gamut_hip_last_error())
        judge([c], hst, st, res, expected, "no second reading, alone")


def test_refused_files_between_good_neighbours(hip, progressive, expected):
    """every file the reference refuses or has no defined result for, each between two good files: refused, the neighbours intact"""
    progressive("device")
    bad = [c for c in CASES if c.verdict != "image"]
    assert len(bad) >= 4
    good = IMAGES[:len(bad) + 1]
    mixed = [good[0]]
    for b, g in zip(bad, good[1:]):
        mixed += [b, g]
    rc, hst, st, res = entropy_decode(hip, [c.data for c in mixed])
    assert rc != 0
    judge(mixed, hst, st, res, expected, "mixed")


@pytest.mark.parametrize("comps", [4, 1])
def test_files_to_pixels(hip, progressive, pixels, comps):
    """the image cases through gamut_hip_jpeg_decode_batch_device: pixels == the oracle's"""
    progressive("device")
    rc, hst, res = _decode_batch_device(hip, [c.data for c in IMAGES], comps)
    assert rc == 0 and not any(hst), (rc, [c.name for c, h in zip(IMAGES, hst) if h], hip.gamut_hip_last_error())
    for c, got in zip(IMAGES, res):
        assert np.array_equal(got, pixels[(c.name, comps)]), (c.name, comps)
