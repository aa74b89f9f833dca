"""The index tables of the decoder images (csrc/nsk_images.h) without a GPU: host/test/images_test.cpp, built by a plain host compiler under
AddressSanitizer + UBSan, builds every table and inverse of decoders 0..3, checks their properties (entries in [-1, total), no parameter twice,
the inverse inverts, the fp32 forward image covers every parameter once, the tail of an image in pieces is the end of its fp32 sibling's
table and shares no parameter with the fragments) and compares one hash line per table with tests/golden/decoder_image_tables.txt, recorded
from the builders as they stood inside nsk.hip.  nsk_decoder_image_table must hand out exactly those tables, and two planted defects in
copies of the header must show."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nice_slam_cpp_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
CSRC = os.path.join(ROOT, "nice-slam-cpp_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "decoder_image_tables.txt")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
LINE = re.compile(r"^(\d) (\d) (\d+) (\d+) (\d+) ([0-9a-f]{16})$", re.M)
_cache = {}


def _recorded():
    with open(TABLE) as f:
        return [line.strip() for line in f if line.strip() and not line.startswith("#")]


def _program_lines():
    if "lines" not in _cache:
        subprocess.check_call(["make", "-s", "-C", HOST, "images_test"])
        r = subprocess.run([os.path.join(HOST, "images_test"), TABLE], capture_output=True, text=True, timeout=120, env=ENV)
        assert r.returncode == 0 and "images_test: 14 tables, 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        _cache["lines"] = [m.group(0) for m in LINE.finditer(r.stdout)]
    return _cache["lines"]


def _fnv1a(table):
    h = 1469598103934665603
    for b in np.ascontiguousarray(table, dtype="<i4").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_the_builders_reproduce_their_recorded_tables():
    lines = _program_lines()
    assert lines == _recorded() and len(lines) == 14              # 4 decoders x 4 images, less the coarse decoder's two images in pieces
    for line in lines:
        which, what, length, n_set, covered = (int(v) for v in line.split()[:5])
        assert n_set == covered <= length                         # no parameter twice
        if what == 0:
            assert covered == pkg.nsk.lib().nsk_decoder_param_count(which)


def test_the_library_hands_out_the_hashed_tables():
    """the table does not depend on the piece count: pieces = 2 and 3 give the same entries (the image's size and layout depend on it)"""
    want = {tuple(int(v) for v in line.split()[:2]): line.split() for line in _program_lines()}
    for which in range(4):
        for what in range(4):
            for pieces in (2, 3):
                t = pkg.nsk.decoder_image_table(which, what, pieces)
                assert t.dtype == np.int32
                if (which, what) not in want:
                    assert which == 0 and what >= 2 and t.size == 0
                    continue
                _, _, length, n_set, _, fnv = want[which, what]
                assert (t.size, int((t >= 0).sum()), _fnv1a(t)) == (int(length), int(n_set), fnv), (which, what, pieces)
    assert np.array_equal(pkg.nsk.decoder_image_table("fine", "fwd16"), pkg.nsk.decoder_image_table(2, 2, 3))


def test_the_entry_point_rejects_bad_arguments():
    L = pkg.nsk.lib()
    buf = (C.c_int32 * 32768)()
    for which, what, pieces in ((-1, 0, 2), (4, 0, 2), (1, -1, 2), (1, 4, 2), (1, 2, 1), (1, 2, 4), (1, 0, 0)):
        assert L.nsk_decoder_image_table(which, what, pieces, buf, 32768) == -1 and b"nsk_decoder_image_table" in L.nsk_last_error(), (which, what, pieces)
    assert L.nsk_decoder_image_table(1, 0, 2, None, 0) == 16100                 # the count alone
    assert L.nsk_decoder_image_table(1, 0, 2, buf, 16099) == -1 and b"capacity" in L.nsk_last_error()
    buf[16100] = 12345
    assert L.nsk_decoder_image_table(1, 0, 2, buf, 16100) == 16100 and buf[16100] == 12345
    assert L.nsk_decoder_image_table(0, 2, 2, buf, 0) == 0 and L.nsk_decoder_image_table(0, 3, 3, None, 0) == 0
    with pytest.raises(pkg.nsk.NskError):
        pkg.nsk.decoder_image_table(1, 2, 5)


PLANTED = {
    # rt and q swapped in seg_fwd: still a permutation of the same parameters, so only the hashes of the fp32 forward images move
    "rt_q_swapped": ("idx[((size_t)(quad0 + rt * KQ + q) * 64 + lane) * 4 + i] = k < kvalid ? Wofs + o * ld + col0 + k : -1;",
                     "idx[((size_t)(quad0 + q * 2 + rt) * 64 + lane) * 4 + i] = k < kvalid ? Wofs + o * ld + col0 + k : -1;"),
    # col0 dropped for W3H: the h part of pts_linear[3] repeats columns of its e part -- parameters twice, others never
    "w3h_col0": ("seg_fwd(idx, I::W3H, 2, L.oW[3], 125, NSK_E, 32);", "seg_fwd(idx, I::W3H, 2, L.oW[3], 125, 0, 32);"),
}


@pytest.mark.parametrize("name", list(PLANTED))
def test_a_planted_defect_shows(name, tmp_path):
    old, new = PLANTED[name]
    with open(os.path.join(CSRC, "nsk_images.h")) as f:
        text = f.read()
    assert text.count(old) == 1
    with open(tmp_path / "nsk_images.h", "w") as f:
        f.write(text.replace(old, new))
    shutil.copy(os.path.join(CSRC, "nsk_layout.h"), tmp_path / "nsk_layout.h")
    exe = str(tmp_path / "images_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I" + str(tmp_path), "-o", exe, os.path.join(HOST, "test", "images_test.cpp")])
    r = subprocess.run([exe, TABLE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "0 failures" not in r.stdout, r.stdout[-3000:]
    good = _program_lines()
    got = [m.group(0) for m in LINE.finditer(r.stdout)]
    if name == "rt_q_swapped":
        assert len(got) == 14 and "appears twice" not in r.stdout
        moved = [g.split()[:2] for g, w in zip(got, good) if g != w]
        assert moved == [[str(w), "0"] for w in range(4)], moved              # and nothing but the hash moved
        assert all(g.split()[:5] == w.split()[:5] for g, w in zip(got, good))
    else:
        assert re.search(r"decoder 1 image 0: parameter \d+ appears twice", r.stdout), r.stdout[-3000:]
        assert "decoder 2 image 0: parameter" in r.stdout and "decoder 3 image 0: parameter" in r.stdout
        assert "decoder 0 image" not in r.stdout                              # the coarse decoder's W3H is another call
