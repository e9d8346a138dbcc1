"""Float64 numpy oracle of the triangle-mesh rasterizer (d3ga_amd/mesh_render.py, csrc/mesh_raster.hip), written from the
semantics section of DESIGN.md 4.4f, and the inputs of its tests.

rasterize_ref is a brute force over every face's pixel bounding box.  Besides the winners it flags the MARGINAL pixels no
float32 implementation can be held to:
  * a pixel where some face whose box contains it has |min(b0, b1, b2)| < EDGE (the pixel centre sits on an edge), and
  * a pixel whose two nearest covering depths differ by less than DEPTH_TIE * zbuf.
Away from them pix_to_face must be exactly the oracle's.  On them the face must be one of the oracle's candidates: a face with
min b >= -EDGE there that is not farther than (1 + DEPTH_TIE) times the nearest face that covers the pixel for certain
(min b >= EDGE); "no face" (-1) is a candidate where no face covers the pixel for certain.
"""
import numpy as np

EDGE = 1e-4
DEPTH_TIE = 1e-5
MARGINAL_CAP = 0.02          # of the covered pixels, in every case
NEAR = 0.01
MIN_AREA = 1e-8

# Value bars: 8 x the largest deviation of the g++ build of csrc/mesh_raster_math.h (-ffp-contract=off, tests/hostcheck/
# meshcheck.cpp) from this oracle on the non-marginal pixels of ALL cases below, rounded up to two digits
# (tests/test_mesh_render_host.py::test_host_build_equals_the_oracle prints the measured values and holds the host build to
# bar / 8).  position and depth in scene units (the scenes span about 1 .. 3), the others dimensionless.
MEASURED = {"bary": 1.8e-4, "zbuf_rel": 4.1e-6, "position": 4.7e-6, "depth": 4.5e-6, "image": 7.0e-5, "normal": 1.3e-7, "vertex_normal": 1.3e-7}
BARS = {k: 8 * v for k, v in MEASURED.items()}


# ---- scenes -------------------------------------------------------------------------------------------------------------
def sphere(nu, nv, seed):
    """A bumpy sphere of radius about 1, open at both poles (the inside shows through the holes: both windings get drawn):
    (nv + 1) rings of nu vertices, F = 2 nu nv faces.  -> (verts (V,3) float32, faces (F,3) int32)"""
    rng = np.random.default_rng(seed)
    theta = np.linspace(0.12, np.pi - 0.12, nv + 1)[:, None]
    phi = (np.arange(nu) * (2 * np.pi / nu))[None, :]
    r = np.ones((nv + 1, nu))
    for _ in range(4):                                        # a few smooth bumps
        a, b = rng.integers(1, 4, 2)
        r = r + 0.02 * rng.standard_normal() * np.cos(a * theta + rng.uniform(0, 6)) * np.cos(b * phi + rng.uniform(0, 6))
    r = r + 0.15 / max(nu, nv) * rng.uniform(-1, 1, r.shape)  # and roughness well below the edge length
    x = np.stack([r * np.sin(theta) * np.cos(phi), r * np.cos(theta) * np.ones_like(phi), r * np.sin(theta) * np.sin(phi)], -1)
    idx = np.arange((nv + 1) * nu).reshape(nv + 1, nu)
    a, b = idx[:-1], np.roll(idx, -1, 1)[:-1]
    c, d = idx[1:], np.roll(idx, -1, 1)[1:]
    faces = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return x.reshape(-1, 3).astype(np.float32), faces.astype(np.int32)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """World-to-camera (R, t) with OpenCV axes (+x right, +y down, +z forward)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(-up, fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return R, -R @ eye


def cam_row(R, t, fx, fy, cx, cy):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64), [fx, fy, cx, cy]]).astype(np.float32)


def _ident(H, W, f):
    return cam_row(np.eye(3), np.zeros(3), f, f * 1.05, 0.5 * W + 0.2, 0.5 * H - 0.1)


def _sphere_cam(H, W, dist, direction, closeup=False):
    d = np.asarray(direction, np.float64)
    R, t = look_at(dist * d / np.linalg.norm(d))
    f = 0.5 * min(H, W) if closeup else 0.45 * min(H, W) * np.sqrt(dist * dist - 1.21) / 1.1
    return cam_row(R, t, f, 1.03 * f, 0.5 * W + 0.3, 0.5 * H - 0.2)


TRI = np.array([[-0.5, -0.3, 2.0], [0.6, -0.2, 2.5], [0.05, 0.45, 1.8]], np.float32)
SMALL = np.array([[-0.62, -0.40, 2.2], [-0.50, -0.40, 2.2], [-0.56, -0.30, 2.2]], np.float32)     # a small triangle up left

# name, nu, nv, seed, H, W, distance, direction, close-up
SPHERES = (("sphere64", 8, 4, 11, 37, 53, 2.2, (0.3, 0.4, -1.0), False),
           ("sphere288", 12, 12, 12, 70, 131, 2.4, (-0.5, 0.2, -1.0), False),
           ("sphere288_closeup", 12, 12, 13, 64, 64, 1.2, (0.2, -0.3, 1.0), True),
           ("sphere5120", 64, 40, 14, 192, 256, 2.6, (1.0, 0.5, 0.4), False),
           ("sphere20000", 100, 100, 15, 96, 128, 2.5, (-0.2, 0.9, 0.6), False))


def make_case(name):
    """-> dict(verts (B,V,3) float32, faces (F,3) int32, cams (B,16) float32, H, W)"""
    one = lambda v, f, cam, H, W: dict(verts=np.ascontiguousarray(v, np.float32)[None], faces=np.asarray(f, np.int32).reshape(-1, 3),
                                       cams=cam[None], H=H, W=W)
    if name == "tri_face0":
        return one(TRI, [[0, 1, 2]], _ident(37, 53, 40.0), 37, 53)
    if name == "tri_face0_flipped":
        return one(TRI, [[0, 2, 1]], _ident(37, 53, 40.0), 37, 53)
    if name == "tri_face1":
        return one(np.concatenate([SMALL, TRI]), [[0, 1, 2], [3, 4, 5]], _ident(37, 53, 40.0), 37, 53)
    if name == "interpenetrating":                            # two triangles that cross along a line, 64 x 64
        v = [[-0.8, -0.6, 1.6], [0.8, -0.5, 2.6], [0.0, 0.7, 2.1], [-0.8, -0.5, 2.6], [0.8, -0.6, 1.6], [0.05, 0.7, 2.0]]
        return one(v, [[0, 1, 2], [3, 4, 5]], _ident(64, 64, 60.0), 64, 64)
    if name == "larger_than_frame":                           # every pixel covered, the box clamped, 15 chunks
        v = [[-30.0, -20.0, 3.0], [30.0, -22.0, 4.0], [1.0, 40.0, 2.0]]
        return one(v, [[0, 1, 2]], _ident(70, 131, 80.0), 70, 131)
    if name == "off_the_sides":                               # one triangle hanging off each side
        v = [[-1.6, -0.1, 2.0], [-0.4, 0.0, 2.2], [-1.5, 0.3, 2.1], [1.5, -0.2, 2.0], [0.5, 0.1, 2.4], [1.7, 0.3, 1.9],
             [-0.1, -1.2, 2.0], [0.2, -0.2, 2.3], [0.3, -1.3, 2.1], [0.0, 1.1, 2.0], [-0.2, 0.25, 2.2], [0.3, 1.4, 1.9]]
        return one(v, [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]], _ident(37, 53, 40.0), 37, 53)
    if name == "one_pixel":
        return one(TRI, [[0, 1, 2]], cam_row(np.eye(3), np.zeros(3), 2.0, 2.0, 0.4, 0.45), 1, 1)
    if name == "three_rows":
        return one(TRI, [[0, 1, 2]], cam_row(np.eye(3), np.zeros(3), 150.0, 5.0, 101.3, 1.4), 3, 200)
    if name in ("sphere64_plus_dropped", "all_dropped"):
        s = [c for c in SPHERES if c[0] == "sphere64"][0]
        v, f = sphere(s[1], s[2], s[3])
        cam = _sphere_cam(s[4], s[5], s[6], s[7])
        R, t = cam[:9].reshape(3, 3).astype(np.float64), cam[9:12].astype(np.float64)
        to_world = lambda p: (R.T @ (np.asarray(p, np.float64) - t)).astype(np.float32)
        n = len(v)
        # a face that crosses the near plane in front of everything, and one of zero area (two equal vertices) nearer than the sphere
        extra = np.stack([to_world([-0.5, -0.5, 0.6]), to_world([0.5, -0.5, 0.6]), to_world([0.0, 0.5, 0.005]),
                          to_world([-0.3, 0.0, 0.8]), to_world([0.3, 0.1, 0.8])])
        v = np.concatenate([v, extra])
        dropped = [[n, n + 1, n + 2], [n + 3, n + 4, n + 4]]
        f = np.array(dropped, np.int32) if name == "all_dropped" else np.concatenate([f, np.array(dropped, np.int32)])
        return one(v, f, cam, s[4], s[5])
    if name == "batch3":                                      # three meshes of one topology, three cameras
        vs, cams = [], []
        for k, (dist, d) in enumerate(((2.2, (0.3, 0.4, -1.0)), (2.5, (-1.0, 0.1, 0.3)), (2.3, (0.1, -0.8, 0.7)))):
            v, f = sphere(8, 4, 21 + k)
            vs.append(v)
            cams.append(_sphere_cam(37, 53, dist, d))
        return dict(verts=np.stack(vs), faces=f, cams=np.stack(cams), H=37, W=53)
    for s in SPHERES:
        if s[0] == name:
            v, f = sphere(s[1], s[2], s[3])
            return one(v, f, _sphere_cam(s[4], s[5], s[6], s[7], s[8]), s[4], s[5])
    raise KeyError(name)


SMALL_CASES = ("tri_face0", "tri_face0_flipped", "tri_face1", "interpenetrating", "larger_than_frame", "off_the_sides", "one_pixel",
               "three_rows", "sphere64_plus_dropped", "batch3")
CASES = SMALL_CASES + tuple(s[0] for s in SPHERES)


def vertex_colours(case, seed=3):
    B, V = case["verts"].shape[:2]
    return np.random.default_rng(seed).random((B, V, 3)).astype(np.float32)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _normalize(v, eps):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), eps)


def rasterize_ref(verts, faces, cam, H, W):
    """One mesh, one camera row; inputs as stored (float32), arithmetic in float64.
    -> dict: pix_to_face (H,W) int, zbuf, bary (perspective-correct) with -1 at background, marginal (H,W) bool, covered
    (pixels with a winner), candidates: sorted int64 codes pixel * (F + 1) + face + 1 of the (pixel, face) pairs allowed on
    marginal pixels (face -1: background), fragments: the number of covering (pixel, face) pairs."""
    v = np.asarray(verts, np.float64)
    cam = np.asarray(cam, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    R, t, (fx, fy, cx, cy) = cam[:9].reshape(3, 3), cam[9:12], cam[12:16]
    vc = v @ R.T + t
    pix = np.full((H, W), -1, np.int64)
    zb = np.full((H, W), -1.0)
    bary = np.full((H, W, 3), -1.0)
    out = dict(pix_to_face=pix, zbuf=zb, bary=bary, marginal=np.zeros((H, W), bool), covered=np.zeros((H, W), bool),
               candidates=np.arange(H * W, dtype=np.int64) * (F + 1), fragments=0)
    if F == 0:
        return out
    z = vc[faces, 2]                                                               # (F,3)
    keep = (z > NEAR).all(1)
    zs = np.where(z > NEAR, z, 1.0)
    x = fx * vc[faces, 0] / zs + cx
    y = fy * vc[faces, 1] / zs + cy
    area = _edge(x[:, 2], y[:, 2], x[:, 0], y[:, 0], x[:, 1], y[:, 1])
    keep &= np.abs(area) >= MIN_AREA
    i0 = np.maximum(np.ceil(x.min(1) - 0.5), 0).astype(np.int64)
    i1 = np.minimum(np.floor(x.max(1) - 0.5), W - 1).astype(np.int64)
    j0 = np.maximum(np.ceil(y.min(1) - 0.5), 0).astype(np.int64)
    j1 = np.minimum(np.floor(y.max(1) - 0.5), H - 1).astype(np.int64)
    w, h = np.maximum(i1 - i0 + 1, 0), np.maximum(j1 - j0 + 1, 0)
    n = np.where(keep, w * h, 0)
    total = int(n.sum())
    if total == 0:
        return out
    fid = np.repeat(np.arange(F), n)
    local = np.arange(total) - np.repeat(np.cumsum(n) - n, n)
    pi, pj = i0[fid] + local % w[fid], j0[fid] + local // w[fid]
    px, py = pi + 0.5, pj + 0.5
    X, Y, A, Z = x[fid], y[fid], area[fid], z[fid]
    b = np.stack([_edge(px, py, X[:, 1], Y[:, 1], X[:, 2], Y[:, 2]), _edge(px, py, X[:, 2], Y[:, 2], X[:, 0], Y[:, 0]),
                  _edge(px, py, X[:, 0], Y[:, 0], X[:, 1], Y[:, 1])], -1) / A[:, None]
    minb = b.min(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        zbuf = 1.0 / (b / Z).sum(1)
    p = pj * W + pi
    marginal = np.zeros(H * W, bool)
    marginal[p[np.abs(minb) < EDGE]] = True
    inside = minb >= 0
    out["fragments"] = int(inside.sum())
    # winners: smallest zbuf, then smallest face index
    sel = np.flatnonzero(inside)
    order = sel[np.lexsort((fid[sel], zbuf[sel], p[sel]))]
    first = np.ones(len(order), bool)
    first[1:] = p[order[1:]] != p[order[:-1]]
    win = order[first]
    pix.reshape(-1)[p[win]] = fid[win]
    zb.reshape(-1)[p[win]] = zbuf[win]
    bp = (b[win] / Z[win]) * zbuf[win, None]
    bary.reshape(-1, 3)[p[win]] = bp
    out["covered"] = pix >= 0
    # the runner-up of every pixel: a depth tie
    second = np.flatnonzero(~first)
    second = second[first[second - 1]]                        # the entry right behind a winner, same pixel
    tie = (zbuf[order[second]] - zbuf[order[second - 1]]) < DEPTH_TIE * zbuf[order[second - 1]]
    marginal[p[order[second[tie]]]] = True
    out["marginal"] = marginal.reshape(H, W)
    # candidates on marginal pixels
    sure = np.full(H * W, np.inf)
    s = np.flatnonzero(minb >= EDGE)
    np.minimum.at(sure, p[s], zbuf[s])
    cand = (minb >= -EDGE) & (zbuf > 0) & (zbuf <= sure[p] * (1 + DEPTH_TIE))
    codes = [p[cand] * (F + 1) + fid[cand] + 1, np.flatnonzero(np.isinf(sure)) * (F + 1)]
    out["candidates"] = np.unique(np.concatenate(codes))
    return out


def check_pix_to_face(ref, got, F):
    """got (H,W) against the oracle: exact away from marginal pixels, a candidate on them.  -> the number of marginal pixels
    where got differs from the oracle's own winner."""
    got = np.asarray(got, np.int64)
    m = ref["marginal"]
    bad = (got != ref["pix_to_face"]) & ~m
    assert not bad.any(), f"{int(bad.sum())} non-marginal pixels with another face, first at {np.argwhere(bad)[0]}"
    codes = np.flatnonzero(m.reshape(-1)) * (F + 1) + got.reshape(-1)[m.reshape(-1)] + 1
    ok = np.isin(codes, ref["candidates"])
    assert ok.all(), f"{int((~ok).sum())} marginal pixels won by a face that is no candidate there"
    return int(((got != ref["pix_to_face"]) & m).sum())


def face_attributes(verts, faces, cam):
    """float64 per-face world positions (F,3,3), face normals (F,3) (clamp 1e-6), view depths (F,3), camera centre."""
    v = np.asarray(verts, np.float64)
    cam = np.asarray(cam, np.float64)
    R, t = cam[:9].reshape(3, 3), cam[9:12]
    fv = v[np.asarray(faces, np.int64)]
    n = _normalize(np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]), 1e-6)
    return fv, n, (v @ R.T + t)[np.asarray(faces, np.int64), 2], -R.T @ t


def shade_ref(verts, faces, cam, pix_to_face, bary, verts_rgb=None, white=True):
    """HardFlatShader at the given fragments (float64) -> (H,W,3)"""
    H, W = pix_to_face.shape
    img = np.full((H, W, 3), 1.0 if white else 0.0)
    m = pix_to_face >= 0
    if not m.any():
        return img
    f = pix_to_face[m]
    bp = np.asarray(bary, np.float64)[m]
    fv, n, _, c = face_attributes(verts, faces, cam)
    rgb = np.ones((len(np.asarray(verts)), 3)) if verts_rgb is None else np.asarray(verts_rgb, np.float64)
    texel = (bp[:, :, None] * rgb[np.asarray(faces, np.int64)[f]]).sum(1)
    p = (bp[:, :, None] * fv[f]).sum(1)
    l = _normalize(c - p, 1e-6)
    cos = (n[f] * l).sum(-1)
    r = 2 * cos[:, None] * n[f] - l
    spec = np.where(cos > 0, np.maximum((l * r).sum(-1), 0.0), 0.0) ** 64
    img[m] = 0.45 * texel + 0.35 * np.maximum(cos, 0)[:, None] * texel + 0.05 * spec[:, None]
    return img


def vertex_normals_ref(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = np.zeros_like(v)
    if len(f):
        c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        for k in range(3):
            np.add.at(n, f[:, k], c)
    return _normalize(n, 1e-6)


def maps_ref(verts, faces, cam, pix_to_face, bary):
    """Renderer.map at the given fragments (float64) -> position (H,W,3), normal (H,W,3), depth (H,W,1), mask (H,W,1)"""
    H, W = pix_to_face.shape
    pos, nrm, depth = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 1))
    mask = (pix_to_face > 0).astype(np.float64)[..., None]
    m = pix_to_face >= 0
    if m.any():
        f = pix_to_face[m]
        bp = np.asarray(bary, np.float64)[m]
        fv, _, fz, _ = face_attributes(verts, faces, cam)
        pos[m] = (bp[:, :, None] * fv[f]).sum(1)
        depth[m] = (bp * fz[f]).sum(1)[:, None]
        vn = vertex_normals_ref(verts, faces)
        nrm[m] = _normalize(vn[np.asarray(faces, np.int64)[f]].sum(1), 1e-8)
    return pos, nrm, depth, mask


class Reference:
    """The oracle's results of one case, element by element, and the checks the host build and the device share."""

    def __init__(self, name):
        self.name = name
        self.case = c = make_case(name)
        self.B, self.V = c["verts"].shape[:2]
        self.F, self.H, self.W = len(c["faces"]), c["H"], c["W"]
        self.rgb = vertex_colours(c)
        self.frag = [rasterize_ref(c["verts"][b], c["faces"], c["cams"][b], self.H, self.W) for b in range(self.B)]

    def marginal_share(self):
        covered = sum(int(f["covered"].sum()) for f in self.frag)
        return sum(int(f["marginal"].sum()) for f in self.frag) / max(covered, 1), covered

    def check_fragments(self, pix, zbuf, bary):
        """(B,H,W), (B,H,W), (B,H,W,3) -> {"bary", "zbuf_rel"}: largest deviations on non-marginal pixels"""
        dev = {"bary": 0.0, "zbuf_rel": 0.0}
        for b, ref in enumerate(self.frag):
            check_pix_to_face(ref, pix[b], self.F)
            bg = np.asarray(pix[b]) < 0
            assert (np.asarray(zbuf[b])[bg] == -1).all() and (np.asarray(bary[b])[bg] == -1).all()
            m = ref["covered"] & ~ref["marginal"]
            if m.any():
                dev["bary"] = max(dev["bary"], float(np.abs(np.asarray(bary[b], np.float64)[m] - ref["bary"][m]).max()))
                dev["zbuf_rel"] = max(dev["zbuf_rel"], float((np.abs(np.asarray(zbuf[b], np.float64)[m] - ref["zbuf"][m]) / ref["zbuf"][m]).max()))
        return dev

    def check_image(self, image, white, coloured):
        """(B,H,W,3) against the shader at the oracle's fragments -> largest deviation on non-marginal pixels (background too)"""
        c, dev = self.case, 0.0
        for b, ref in enumerate(self.frag):
            want = shade_ref(c["verts"][b], c["faces"], c["cams"][b], ref["pix_to_face"], ref["bary"], self.rgb[b] if coloured else None, white)
            m = ~ref["marginal"]
            bg = m & ~ref["covered"]
            assert (np.asarray(image[b])[bg] == (1.0 if white else 0.0)).all()
            dev = max(dev, float(np.abs(np.asarray(image[b], np.float64)[m] - want[m]).max()))
        return dev

    def check_maps(self, pos, nrm, depth, mask):
        c, dev = self.case, {"position": 0.0, "normal": 0.0, "depth": 0.0}
        for b, ref in enumerate(self.frag):
            want = maps_ref(c["verts"][b], c["faces"], c["cams"][b], ref["pix_to_face"], ref["bary"])
            m = ~ref["marginal"]
            assert np.array_equal(np.asarray(mask[b])[m], want[3][m].astype(np.float32)), "mask"
            for k, got in (("position", pos), ("normal", nrm), ("depth", depth)):
                g = np.asarray(got[b], np.float64)
                assert (g[m & ~ref["covered"]] == 0).all(), k
                dev[k] = max(dev[k], float(np.abs(g[m] - want[("position", "normal", "depth").index(k)][m]).max()))
        return dev

    def check_vertex_normals(self, normals):
        c = self.case
        return max(float(np.abs(np.asarray(normals[b], np.float64) - vertex_normals_ref(c["verts"][b], c["faces"])).max()) for b in range(self.B))


_REFS = {}


def reference(name):
    """The oracle of a case, computed once per process."""
    if name not in _REFS:
        _REFS[name] = Reference(name)
    return _REFS[name]
