"""Shared by tests/test_sfm_cpu.py and tests/test_gpu_sfm.py (not a test module): synthetic structure-from-motion models, writers
of COLMAP's text and binary layouts, the view graph restated in NumPy with arccos / exp, the host build
of mvster_amd/csrc/sfm_math.h, and the case arrays.

Neither yardstick comes from the reference tree, which has no such step: the restatement follows the definition in float64 with
NumPy's own arccos and exp, the host build is the kernels' own arithmetic compiled for the CPU."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np

from mvster_amd import sfm
from tests import fusion_scene_cases as C

TWO32 = 4294967296.0


# ---- synthetic models ---------------------------------------------------------------------------------------------------------

def quaternion_of(R):
    """A rotation matrix -> the unit quaternion (w, x, y, z) with w >= 0 (Shepperd's choice of the largest component)."""
    t = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(t))
    if k == 0:
        w = 0.5 * np.sqrt(1 + t[0])
        q = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]
    elif k == 1:
        x = 0.5 * np.sqrt(1 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)]
    elif k == 2:
        y = 0.5 * np.sqrt(1 - R[0, 0] + R[1, 1] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / (4 * y), (R[0, 1] + R[1, 0]) / (4 * y), y, (R[1, 2] + R[2, 1]) / (4 * y)]
    else:
        z = 0.5 * np.sqrt(1 - R[0, 0] - R[1, 1] + R[2, 2])
        q = [(R[1, 0] - R[0, 1]) / (4 * z), (R[0, 2] + R[2, 0]) / (4 * z), (R[1, 2] + R[2, 1]) / (4 * z), z]
    q = np.array(q, dtype=np.float64)
    return -q if q[0] < 0 else q


def look_at(centre, target):
    """World-to-camera rotation of a camera at ``centre`` looking at ``target`` (x right, y down, z forward)."""
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def synthetic_model(V=24, P=600, seed=0, rings=2, dropout=0.3, width=160, height=120, focal=140.0, id_step=1, repeat=0.0,
                    orphans=0.0, unmatched=0.2, model=1):
    """Cameras on ``rings`` rings around a point set looking at its middle; a view sees a point that projects inside its image
    unless ``dropout`` strikes.  -> the raw model the writers take: ``cameras`` {id: (model id, w, h, params)}, ``images`` [(id,
    qvec, tvec, camera id, name, points2D [n,3] = x, y, point id)], ``points`` [(id, xyz, rgb, error, track)].  ``id_step``:
    image ids are 1, 1 + id_step, ...; ``repeat``: the share of observations written twice; ``orphans``: of observations naming
    a point id the points file does not hold; ``unmatched``: extra observations with id -1 per matched one."""
    rng = np.random.RandomState(seed)
    pts = (rng.rand(P, 3) - 0.5) * np.array([4.0, 4.0, 2.0])
    point_ids = np.sort(rng.choice(np.arange(1, 3 * P + 1), P, replace=False)).astype(np.int64)
    params = {0: [focal, width / 2, height / 2], 1: [focal, focal * 1.01, width / 2, height / 2],
              2: [focal, width / 2, height / 2, 0.0], 3: [focal, width / 2, height / 2, 0.0, 0.0],
              4: [focal, focal, width / 2, height / 2, 0.0, 0.0, 0.0, 0.0]}[model]
    cameras = {3: (model, width, height, params)}
    fx, fy, cx, cy = (params[0], params[1], params[2], params[3]) if model in (1, 4) else (params[0], params[0], params[1], params[2])
    images, tracks = [], {int(i): [] for i in point_ids}
    for v in range(V):
        ring = v % rings
        ang = 2 * np.pi * (v // rings) / max(1, (V + rings - 1) // rings) + 0.3 * ring
        centre = np.array([np.cos(ang), np.sin(ang), 0.0]) * (6.0 + 1.5 * ring) + np.array([0.0, 0.0, 1.0 + 2.0 * ring])
        R = look_at(centre, rng.randn(3) * 0.2)
        q = quaternion_of(R)
        t = -R @ centre
        cam = pts @ R.T + t
        u, w = fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy
        seen = (cam[:, 2] > 0) & (u >= 0) & (u < width) & (w >= 0) & (w < height) & (rng.rand(P) >= dropout)
        rows = [(u[p], w[p], int(point_ids[p])) for p in np.nonzero(seen)[0]]
        rows += [r for r in rows if rng.rand() < repeat]
        rows += [(rng.rand() * width, rng.rand() * height, int(3 * P + 7 + k)) for k in range(int(orphans * len(rows)))]
        rows += [(rng.rand() * width, rng.rand() * height, -1) for _ in range(int(unmatched * len(rows)))]
        rows = [rows[k] for k in rng.permutation(len(rows))]
        image_id = 1 + v * id_step
        for k, r in enumerate(rows):
            if r[2] in tracks:
                tracks[r[2]].append((image_id, k))
        images.append((image_id, q, t, 3, "view %03d.png" % v if v % 5 == 0 else "ring%d/view_%03d.png" % (ring, v),
                       np.array(rows, dtype=np.float64).reshape(-1, 3)))
    points = [(int(point_ids[p]), pts[p], rng.randint(0, 256, 3), float(rng.rand()), tracks[int(point_ids[p])]) for p in range(P)]
    order = rng.permutation(V)                                                  # (the files are not in id order)
    return dict(cameras=cameras, images=[images[k] for k in order], points=[points[k] for k in rng.permutation(P)])


def write_text(raw, path, comments=True):
    os.makedirs(path, exist_ok=True)
    note = (lambda s: "# %s\n" % s) if comments else (lambda s: "")
    with open(os.path.join(path, "cameras.txt"), "w") as f:
        f.write(note("Camera list with one line of data per camera:") + note("  CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]"))
        for cid, (model, w, h, params) in sorted(raw["cameras"].items()):
            f.write("%d %s %d %d %s\n" % (cid, sfm.CAMERA_MODELS[model][0] if model in sfm.CAMERA_MODELS else "FULL_OPENCV", w, h,
                                          " ".join(repr(float(p)) for p in params)))
    with open(os.path.join(path, "images.txt"), "w") as f:
        f.write(note("Image list with two lines of data per image:") + note("  IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME"))
        for k, (iid, q, t, cid, name, obs) in enumerate(raw["images"]):
            if comments and k == 2:
                f.write("# a comment between two images\n")
            f.write("%d %s %s %d %s\n" % (iid, " ".join(repr(float(x)) for x in q), " ".join(repr(float(x)) for x in t), cid, name))
            f.write(" ".join("%r %r %d" % (float(x), float(y), int(p)) for x, y, p in obs) + "\n")
    with open(os.path.join(path, "points3D.txt"), "w") as f:
        f.write(note("3D point list with one line of data per point:"))
        for pid, xyz, rgb, err, track in raw["points"]:
            f.write("%d %s %d %d %d %r %s\n" % (pid, " ".join(repr(float(x)) for x in xyz), rgb[0], rgb[1], rgb[2], err,
                                                " ".join("%d %d" % t for t in track)))


def write_binary(raw, path):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(raw["cameras"])))
        for cid, (model, w, h, params) in sorted(raw["cameras"].items()):
            f.write(struct.pack("<iiQQ", cid, model, w, h) + struct.pack("<%dd" % len(params), *params))
    with open(os.path.join(path, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(raw["images"])))
        for iid, q, t, cid, name, obs in raw["images"]:
            f.write(struct.pack("<i7di", iid, *[float(x) for x in q], *[float(x) for x in t], cid) + name.encode("utf-8") + b"\0")
            f.write(struct.pack("<Q", len(obs)))
            for x, y, p in obs:
                f.write(struct.pack("<ddq", float(x), float(y), int(p)))
    with open(os.path.join(path, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(raw["points"])))
        for pid, xyz, rgb, err, track in raw["points"]:
            f.write(struct.pack("<Q3d3BdQ", pid, *[float(x) for x in xyz], int(rgb[0]), int(rgb[1]), int(rgb[2]), err, len(track)))
            for t in track:
                f.write(struct.pack("<ii", *t))


def write_images(raw, path, seed=0):
    """An 8-bit PNG per image of the raw model, at its camera's size -> {name: uint8 [H,W,3]}"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = {}
    for iid, q, t, cid, name, obs in raw["images"]:
        _, w, h, _ = raw["cameras"][cid]
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        os.makedirs(os.path.dirname(os.path.join(path, name)), exist_ok=True)
        Image.fromarray(img).save(os.path.join(path, name))
        out[name] = img
    return out


def arrays_of(model):
    """The kernels' inputs of a model (``sfm.read_sfm_model``) -> dict"""
    return dict(centres=np.ascontiguousarray(model["centres"]), points=np.ascontiguousarray(model["points"]),
                rt=sfm.depth_rows(model), view_ptr=model["view_ptr"], view_pts=model["view_pts"], pt_ptr=model["pt_ptr"],
                pt_views=model["pt_views"])


def arrays_from(centres, points, rt, view_of_obs, point_of_obs):
    centres, points = np.ascontiguousarray(centres, np.float64).reshape(-1, 3), np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    out = dict(centres=centres, points=points, rt=np.ascontiguousarray(rt, np.float64).reshape(-1, 4))
    out.update(sfm.structure(view_of_obs, point_of_obs, len(centres), len(points)))
    return out


# ---- the definition, restated ----------------------------------------------------------------------------------------------------

def common_counts(a):
    """n_common [V,V] int64: the points two views share (the diagonal: a view's own points)"""
    V, P = len(a["centres"]), len(a["points"])
    M = np.zeros((V, P), np.int64)
    M[np.repeat(np.arange(V), np.diff(a["view_ptr"])), a["view_pts"]] = 1
    return M @ M.T


def pair_scores_numpy(a, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """q [V,V] uint64 with NumPy's arccos and exp in float64: per point all pairs of its track at once."""
    V = len(a["centres"])
    q = np.zeros((V, V), np.uint64)
    for p in range(len(a["points"])):
        views = a["pt_views"][a["pt_ptr"][p]:a["pt_ptr"][p + 1]]
        if len(views) < 2:
            continue
        d = a["centres"][views] - a["points"][p]
        nn = (d * d).sum(1)
        i, j = np.triu_indices(len(views), 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = (d[i] * d[j]).sum(1) / np.sqrt(nn[i] * nn[j])
            theta = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
            sigma = np.where(theta <= theta0, sigma1, sigma2)
            term = np.exp(-(theta - theta0) ** 2 / (2 * sigma ** 2))
        term[~((nn[i] > 0) & (nn[j] > 0))] = 0.0
        np.add.at(q, (views[i], views[j]), np.floor(term * TWO32 + 0.5).astype(np.uint64))
    return q + q.T


def depth_ranges_numpy(a):
    V = len(a["rt"])
    n, lo, hi = np.zeros(V, np.int32), np.full(V, np.nan), np.full(V, np.nan)
    for v in range(V):
        x = a["points"][a["view_pts"][a["view_ptr"][v]:a["view_ptr"][v + 1]]]
        r = a["rt"][v]
        with np.errstate(invalid="ignore"):
            z = ((r[0] * x[:, 0] + r[1] * x[:, 1]) + r[2] * x[:, 2]) + r[3]
            z = np.sort(z[np.isfinite(z) & (z > 0)])
        n[v] = len(z)
        if len(z):
            lo[v], hi[v] = z[len(z) // 100], z[99 * len(z) // 100]
    return n, lo, hi


def select_numpy(q, num_src):
    """-> index [V,num_src] int32, value [V,num_src] uint64, count [V] int32 by np.lexsort on (j, -q)"""
    V = len(q)
    index, value, count = np.full((V, num_src), -1, np.int32), np.zeros((V, num_src), np.uint64), np.zeros(V, np.int32)
    for i in range(V):
        row = q[i].astype(np.uint64).copy()
        row[i] = 0
        order = np.lexsort((np.arange(V), np.iinfo(np.uint64).max - row))       # q descending, then j ascending
        order = [j for j in order if row[j] > 0][:num_src]
        count[i] = len(order)
        index[i, :len(order)] = order
        value[i, :len(order)] = row[order]
    return index, value, count


# ---- the host build of mvster_amd/csrc/sfm_math.h --------------------------------------------------------------------------------

_HM = {}


def load_sfm_hostmath(compilers=("g++",)):
    """Compile tests/hostmath/sfm_hostmath.cpp with the flags of ``fusion_scene_cases.load_geo_hostmath`` and load it, once per
    process.  No compiler is an error, never a skip."""
    if compilers in _HM:
        return _HM[compilers]
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (shutil.which(n) or (os.path.join(rocm, "llvm", "bin", n) if n == "clang++" else None)
                         for n in compilers) if c and os.path.exists(c)]
    if not found:
        raise RuntimeError("no host C++ compiler among %s: the host build of sfm_math.h cannot be made" % (compilers,))
    so = os.path.join(C.HOSTMATH, "libsfmhostmath.so")
    subprocess.check_call([found[0]] + C.HOST_FLAGS + ["-o", so, os.path.join(C.HOSTMATH, "sfm_hostmath.cpp")])
    h = ctypes.CDLL(so)
    p, l, i, d = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double
    h.hm_sfm_pair_scores.restype, h.hm_sfm_pair_scores.argtypes = None, [p, i, p, l, p, p, d, d, d, p]
    h.hm_sfm_depth_ranges.restype, h.hm_sfm_depth_ranges.argtypes = None, [p, i, p, p, p, p, p, p]
    h.hm_sfm_select_sources.restype, h.hm_sfm_select_sources.argtypes = None, [p, i, i, p, p, p]
    h.hm_sfm_terms.restype, h.hm_sfm_terms.argtypes = None, [p, p, p, l, d, d, d, p, p, p, p]
    h.hm_sfm_pairs.restype, h.hm_sfm_pairs.argtypes = None, [l, p]
    h.hm_sfm_pair_at.restype, h.hm_sfm_pair_at.argtypes = None, [l, l, p]
    h.hm_sfm_exp_neg.restype, h.hm_sfm_exp_neg.argtypes = d, [d]
    _HM[compilers] = h
    return h


def pair_scores_host(h, a, theta0=5.0, sigma1=1.0, sigma2=10.0):
    V = len(a["centres"])
    q = np.zeros((V, V), np.uint64)
    pt_ptr, pt_views = np.ascontiguousarray(a["pt_ptr"], np.int64), np.ascontiguousarray(a["pt_views"], np.int32)
    h.hm_sfm_pair_scores(a["centres"].ctypes.data, V, a["points"].ctypes.data, len(a["points"]), pt_ptr.ctypes.data,
                         pt_views.ctypes.data, theta0, sigma1, sigma2, q.ctypes.data)
    return q


def depth_ranges_host(h, a):
    V = len(a["rt"])
    n, lo, hi = np.zeros(V, np.int32), np.zeros(V, np.float64), np.zeros(V, np.float64)
    view_ptr, view_pts = np.ascontiguousarray(a["view_ptr"], np.int64), np.ascontiguousarray(a["view_pts"], np.int32)
    h.hm_sfm_depth_ranges(a["rt"].ctypes.data, V, a["points"].ctypes.data, view_ptr.ctypes.data, view_pts.ctypes.data,
                          n.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    return n, lo, hi


def select_host(h, q, num_src):
    q = np.ascontiguousarray(q).view(np.uint64)
    V = len(q)
    index, value, count = np.zeros((V, num_src), np.int32), np.zeros((V, num_src), np.uint64), np.zeros(V, np.int32)
    h.hm_sfm_select_sources(q.ctypes.data, V, num_src, index.ctypes.data, value.ctypes.data, count.ctypes.data)
    return index, value, count


def terms_host(h, ci, cj, x, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """-> dict(term, theta, qterm, err): the header's term of every triple and its difference from long double libm"""
    ci, cj, x = (np.ascontiguousarray(v, np.float64).reshape(-1, 3) for v in (ci, cj, x))
    n = len(ci)
    term, theta, qterm, err = np.zeros(n), np.zeros(n), np.zeros(n, np.uint64), np.zeros(n)
    h.hm_sfm_terms(ci.ctypes.data, cj.ctypes.data, x.ctypes.data, n, theta0, sigma1, sigma2, term.ctypes.data, theta.ctypes.data,
                   qterm.ctypes.data, err.ctypes.data)
    return dict(term=term, theta=theta, qterm=qterm, err=err)


def graph_host(h, a, theta0=5.0, sigma1=1.0, sigma2=10.0, num_src=10):
    """The dict of ``sfm.view_graph`` from the host build."""
    q = pair_scores_host(h, a, theta0, sigma1, sigma2)
    index, value, count = select_host(h, q, num_src)
    n, lo, hi = depth_ranges_host(h, a)
    out = dict(q=q.view(np.int64), score=q.astype(np.float64) / TWO32, src_index=index, src_q=value.view(np.int64), src_count=count,
               n_obs=n, depth_min=lo, depth_max=hi)
    out["pairs"], out["pair_scores"] = sfm.source_lists(index, out["src_q"], count)
    return out


def assert_bytes(g, w, what=""):
    g, w = np.asarray(g), np.asarray(w)
    assert g.dtype.itemsize == w.dtype.itemsize and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.nonzero(np.frombuffer(g.tobytes(), np.uint8) != np.frombuffer(w.tobytes(), np.uint8))[0]
        k = int(bad[0]) // g.dtype.itemsize
        raise AssertionError((what, "%d bytes differ, the first in element %d: %r against %r" % (len(bad), k, g.ravel()[k], w.ravel()[k])))


# ---- the case arrays ---------------------------------------------------------------------------------------------------------

def ring_centres(V, radius=8.0, seed=0):
    rng = np.random.RandomState(seed)
    ang = 2 * np.pi * np.arange(V) / V
    return np.stack([radius * np.cos(ang), radius * np.sin(ang), 1.0 + 0.5 * rng.rand(V)], 1)


def rows_at(centres, target=(0.0, 0.0, 0.0)):
    """rt [V,4] of cameras at ``centres`` looking at ``target``"""
    out = []
    for c in np.asarray(centres, np.float64):
        R = look_at(c, np.asarray(target, np.float64) + 1e-3)
        out.append(np.concatenate([R[2], [-(R @ c)[2]]]))
    return np.array(out)


TRACK_LENGTHS = (1, 2, 64, 65, 300)


def track_case(V=301, seed=1):
    """Tracks of length 1, 2, 64, 65 and 300 (four points each, shuffled) over V - 1 = 300 views on a ring; the last view
    observes nothing.  The work items of a track of 300 (44 850) cross wave and workgroup boundaries, and its last item is the
    largest triangular index."""
    rng = np.random.RandomState(seed)
    centres = ring_centres(V, seed=seed)
    lengths = rng.permutation(np.repeat(TRACK_LENGTHS, 4))
    points = (rng.rand(len(lengths), 3) - 0.5) * 3.0
    vo, po = [], []
    for p, L in enumerate(lengths):
        views = rng.choice(V - 1, L, replace=False)
        vo += list(views)
        po += [p] * L
    return arrays_from(centres, points, rows_at(centres), vo, po), lengths


def two_view_case():
    centres = np.array([[4.0, 0.0, 1.0], [3.9, 0.6, 1.0]])
    points = np.array([[0.1, 0.2, 0.0], [-0.3, 0.1, 0.4], [0.0, 0.0, -0.2]])
    return arrays_from(centres, points, rows_at(centres), [0, 0, 0, 1, 1], [0, 1, 2, 0, 2])


def term_case():
    """Views 0 / 1 share a centre (theta = 0 on every point), views 0 / 2 lie opposite each other about point 0 (theta = 180),
    point 1 sits at the centre of view 3, point 2 is observed twice by views 0 and 4, and views 4 / 5 see point 3 under some
    angle which the tests also pass as theta0 (theta exactly theta0)."""
    centres = np.array([[5.0, 1.0, 0.5], [5.0, 1.0, 0.5], [-5.0, -1.0, -0.5], [2.0, -3.0, 1.0], [4.0, 2.0, 1.0], [4.2, 1.5, 1.1]])
    points = np.array([[0.0, 0.0, 0.0], [2.0, -3.0, 1.0], [0.3, 0.1, -0.2], [0.05, -0.1, 0.2]])
    vo = [0, 1, 2, 3, 4, 5,  0, 3, 4,  0, 0, 4, 4, 1,  4, 5]
    po = [0, 0, 0, 0, 0, 0,  1, 1, 1,  2, 2, 2, 2, 2,  3, 3]
    return arrays_from(centres, points, rows_at(centres), vo, po)


DEPTH_COUNTS = (1, 2, 99, 100, 101, 257)


def depth_case(seed=2):
    """Views with the identity's third row (z is the point's own z): n = 1, 2, 99, 100, 101, 257 valid depths (views 0 .. 5),
    all-equal depths (6), negative, zero, inf and NaN depths mixed in (7), 256 depths that share their top 56 bits (8) and a
    view that sees only invalid depths (9).  -> (arrays, expected n)"""
    rng = np.random.RandomState(seed)
    zs, vo = [], []
    for v, n in enumerate(DEPTH_COUNTS):
        zs += list(1.0 + 9.0 * rng.rand(n))
        vo += [v] * n
    zs += [3.25] * 37
    vo += [6] * 37
    mixed = list(0.5 + rng.rand(150)) + [-1.0, -0.0, 0.0, np.inf, -np.inf, np.nan, -2.5e-300, 5e-324] * 4
    mixed = [mixed[k] for k in rng.permutation(len(mixed))]
    zs += mixed
    vo += [7] * len(mixed)
    base = np.float64(2.7182818).view(np.uint64) & ~np.uint64(255)
    near = (base + rng.permutation(256).astype(np.uint64)).view(np.float64)
    zs += list(near)
    vo += [8] * 256
    zs += [np.nan, -1.0, 0.0, np.inf]
    vo += [9] * 4
    zs = np.array(zs, dtype=np.float64)
    points = np.stack([rng.rand(len(zs)), rng.rand(len(zs)), zs], 1)
    V = 10
    rt = np.tile(np.array([0.0, 0.0, 1.0, 0.0]), (V, 1))
    centres = ring_centres(V, seed=seed)
    a = arrays_from(centres, points, rt, vo, np.arange(len(zs)))
    return a, np.array(list(DEPTH_COUNTS) + [37, 150 + 4, 256, 0], dtype=np.int32)     # (5e-324 > 0 is kept: 4 of them)


def select_matrix(V, seed, density=0.5, levels=None):
    """A symmetric int64 [V,V] matrix with a zero diagonal; ``levels``: draw the scores from so few values that many are equal."""
    rng = np.random.RandomState(seed)
    q = rng.randint(1, 1 << 40, size=(V, V)).astype(np.int64) if levels is None else rng.randint(1, levels + 1, size=(V, V)).astype(np.int64)
    q[rng.rand(V, V) >= density] = 0
    q = np.triu(q, 1)
    return np.ascontiguousarray(q + q.T)
