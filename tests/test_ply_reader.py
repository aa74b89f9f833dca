"""CPU tests (-m "not gpu") of Mesher::read_ply_mesh through host/ply_test: PLY files this project did not write.  Every file is written here."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")

VERTS = np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, -0.25], [0.5, 1.5, 2], [0.1, 0.2, 0.3]], np.float64)
FACES = [[0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 4, 3], [5, 4]]
TRIS = [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 4], [0, 4, 3]]          # fans; the two-corner face is dropped
FMT = {"char": "b", "uchar": "B", "short": "h", "ushort": "H", "int": "i", "uint": "I", "float": "f", "double": "d",
       "int8": "b", "uint8": "B", "int16": "h", "uint16": "H", "int32": "i", "uint32": "I", "float32": "f", "float64": "d"}


@pytest.fixture(scope="module")
def exe():
    import nice_slam_cpp_amd as pkg
    pkg.build()
    subprocess.check_call(["make", "-s", "-C", HOST, "ply_test"])
    return os.path.join(HOST, "ply_test")


def write_ply(path, ascii_, vprops, count_type="uchar", index_type="int", verts=VERTS, faces=FACES, fmt=None, extra_element=False,
              face_scalar_first=False, crlf=False):
    """vprops: list of (name, type); x, y, z take the coordinates, any other property the value 7"""
    nl = "\r\n" if crlf else "\n"
    h = ["ply", "format %s 1.0" % (fmt or ("ascii" if ascii_ else "binary_little_endian")), "comment written by the test"]
    if extra_element:
        h += ["element camera 2", "property float focal", "property list uchar short pix"]
    h += ["element vertex %d" % len(verts)] + ["property %s %s" % (t, n) for n, t in vprops]
    h += ["element face %d" % len(faces)] + (["property uchar flag"] if face_scalar_first else []) + ["property list %s %s vertex_indices" % (count_type, index_type),
                                                                                                "property float quality"]
    h += ["end_header"]
    rows = []                                               # (type, value) in file order
    if extra_element:
        for k in range(2):
            rows += [[("float", 1.5), ("uchar", 2), ("short", -3), ("short", 4)]]
    for p in verts:
        rows.append([(t, float(p["xyz".index(n)]) if n in ("x", "y", "z") else 7) for n, t in vprops])
    for fc in faces:
        rows.append(([("uchar", 1)] if face_scalar_first else []) + [(count_type, len(fc))] + [(index_type, i) for i in fc] + [("float", 0.5)])
    with open(path, "wb") as f:
        f.write((nl.join(h) + nl).encode())
        for r in rows:
            if ascii_:
                f.write((" ".join(repr(v) if isinstance(v, float) else str(v) for _, v in r) + nl).encode())
            else:
                for t, v in r:
                    f.write(struct.pack("<" + FMT[t], v if FMT[t] in "fd" else int(v)))


def read_all(exe, paths):
    """one run of ply_test over all the files -> {path: (verts float32, tris) or the reader's message}"""
    out = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    res, lines, k = {}, out.stdout.split("\n"), 0
    while k < len(lines) and lines[k].startswith("file "):
        path = lines[k][5:]
        if lines[k + 1].startswith("error "):
            res[path] = lines[k + 1][6:]; k += 2
            continue
        nv, nt = map(int, lines[k + 1].split())
        v = np.array([l.split() for l in lines[k + 2:k + 2 + nv]], np.float64).astype(np.float32).reshape(nv, 3)      # (%.9g round-trips a float32)
        t = np.array([l.split() for l in lines[k + 2 + nv:k + 2 + nv + nt]], np.int64).reshape(nt, 3)
        res[path] = (v, t); k += 2 + nv + nt
    assert len(res) == len(paths)
    return res


XYZ = [("x", "float"), ("y", "float"), ("z", "float")]
LAYOUTS = {
    "plain": XYZ,
    "extras_around": [("nx", "float"), ("confidence", "uchar")] + XYZ + [("red", "uchar"), ("green", "uchar"), ("blue", "uchar"), ("w", "double")],
    "doubles": [("x", "double"), ("y", "double"), ("z", "double")],
    "shuffled": [("z", "float32"), ("s", "int16"), ("y", "float64"), ("x", "float"), ("k", "uint")],
}


TYPES = [("uchar", "int"), ("uchar", "uint"), ("ushort", "ushort"), ("int", "uchar"), ("uint8", "int32")]


def test_header_driven_reading(exe, tmp_path):
    """ascii and binary; extra vertex properties before and after x y z, in any order and type; double coordinates; every count / index type;
    a triangle, a quad, a pentagon and a two-corner face; another element before the vertices; a scalar face property; CR LF line ends"""
    paths = []
    for ascii_ in (True, False):
        for layout in sorted(LAYOUTS):
            for ct, it in TYPES:
                p = tmp_path / ("%s_%s_%s_%s.ply" % ("a" if ascii_ else "b", layout, ct, it))
                write_ply(p, ascii_, LAYOUTS[layout], ct, it, extra_element=layout == "shuffled", face_scalar_first=layout == "doubles",
                          crlf=ascii_ and layout == "plain")
                paths.append(p)
    own = tmp_path / "own.ply"
    tris = np.array(TRIS[:3], np.int32)
    with open(own, "wb") as f:               # what Mesher::write_ply writes
        f.write(("ply\nformat binary_little_endian 1.0\ncomment nice-slam-cpp_amd Mesher\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                 "property list uchar int vertex_indices\nend_header\n" % (len(VERTS), len(tris))).encode())
        for q in VERTS:
            f.write(struct.pack("<fffBBB", *q, 1, 2, 3))
        for q in tris:
            f.write(struct.pack("<Biii", 3, *q))
    res = read_all(exe, paths + [own])
    for p in paths:
        v, t = res[str(p)]
        assert (v == VERTS.astype(np.float32)).all(), p
        assert t.tolist() == TRIS, p
    v, t = res[str(own)]
    assert (v == VERTS.astype(np.float32)).all() and t.tolist() == TRIS[:3]


def test_errors_carry_the_path(exe, tmp_path):
    want = {}                                   # path -> a word the message must hold
    for ascii_ in (True, False):
        tag = "a_" if ascii_ else "b_"
        good = tmp_path / (tag + "good.ply")
        write_ply(good, ascii_, LAYOUTS["extras_around"])
        data = open(good, "rb").read()
        body = data.index(b"end_header\n") + 11
        for name, cut in (("cut_faces", len(data) - 3 if not ascii_ else len(data) - 12), ("cut_vertices", body + 20), ("cut_header", body - 15)):
            p = tmp_path / (tag + name + ".ply")
            open(p, "wb").write(data[:cut])
            want[p] = "truncated"
        p = tmp_path / (tag + "range.ply"); write_ply(p, ascii_, XYZ, faces=[[0, 1, 2], [0, 1, len(VERTS)]]); want[p] = "outside"
        p = tmp_path / (tag + "negative.ply"); write_ply(p, ascii_, XYZ, faces=[[0, -1, 2]]); want[p] = "outside"
        p = tmp_path / (tag + "big.ply"); write_ply(p, ascii_, XYZ, fmt="binary_big_endian"); want[p] = "big-endian"
        p = tmp_path / (tag + "noxyz.ply"); write_ply(p, ascii_, [("x", "float"), ("y", "float"), ("q", "float")]); want[p] = "x, y, z"
    want[tmp_path / "absent.ply"] = "cannot open"
    open(tmp_path / "not.ply", "wb").write(b"solid\nfacet\n"); want[tmp_path / "not.ply"] = "not a PLY"
    res = read_all(exe, list(want))
    for p, word in want.items():
        msg = res[str(p)]
        assert isinstance(msg, str) and str(p) in msg and word in msg, (p, msg)
