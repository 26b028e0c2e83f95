"""Scenes that turn the light lists' cube map (csrc/rt_lists.h "Light lists"): a closed room around a
one-point light with sparse occluders in every direction, and one small scene per geometry class of the
binning kernels.  Plain module: no pytest here.  tests/test_light_list_cases_cpu.py validates the fixtures
on the oracle alone, tests/test_light_list_directions.py renders them on the GPU.

The room is a box of 12 inward-facing triangles, 10 units a side.  The light is a small one-face
triangle whose vertex 0 -- the sample point P of quirk S2 -- sits a little off the room's middle.  The
occluders sit on a Fibonacci lattice of directions around P at radius 1 to 3; each has an angular radius of
0.06 to 0.09 rad (four to six cells of the 128 x 128 faces) against a lattice spacing of 0.3 rad, so no
two overlap seen from P and every one casts a shadow of its own on a wall.  Six cameras, one in front of each
wall, look at the opposite wall: together their hit points see P from every side.

Every check here is a statement about the reference (ol.oracle_render, ray_oracle): whether a fixture
does what it was built for never depends on the code under test.
"""
import functools

import numpy as np

import oracle_lib as ol
import ray_oracle as ro

F32 = np.float32
HALF = 5.0          # the room's half side
W = H = 96          # frame size of every view
P_OFF = np.array([0.03, -0.02, 0.05])  # P relative to the room's middle: on no plane of symmetry
FACE_NAMES = ("+x", "-x", "+y", "-y", "+z", "-z")  # rt_lists.h light_list_cell: 2 * axis + (negative)

WALL_COLOURS = [(0.7, 0.3, 0.3), (0.3, 0.7, 0.3), (0.3, 0.3, 0.7), (0.7, 0.7, 0.3), (0.3, 0.7, 0.7), (0.7, 0.3, 0.7)]


def _mat(c):
    return ol.material13(ka=c, kd=c)


# ---- pieces -------------------------------------------------------------------------------------------
def room_walls(c):
    """six geometries of two triangles, normals cross(v1 - v0, v2 - v0) pointing into the room"""
    c = np.asarray(c, float)
    geoms = []
    for m in range(3):
        for s in (1.0, -1.0):
            a, b = (m + 1) % 3, (m + 2) % 3
            q = np.zeros((4, 3))
            q[:, m] = s * HALF
            q[:, a] = (-HALF, HALF, HALF, -HALF)
            q[:, b] = (-HALF, -HALF, HALF, HALF)
            tris = q[[0, 1, 2, 0, 2, 3]] if s < 0 else q[[0, 2, 1, 0, 3, 2]]
            n = np.cross(tris[1] - tris[0], tris[2] - tris[0])
            assert n[m] * s < 0, "wall normal must point inwards"
            geoms.append({"vertex": (tris + c).astype(F32), "face_index": np.arange(6).reshape(2, 3),
                          "material": _mat(WALL_COLOURS[len(geoms)])})
    return geoms


def light_triangles(p, n_faces=1, size=0.06):
    """a light of n_faces faces; its sample points are vertex 0 .. n_faces - 1 (quirk S2)"""
    p = np.asarray(p, float)
    v = [p, p + (size, 0.0, 0.2 * size), p + (0.0, 0.3 * size, size)]
    if n_faces == 2:  # the second sample point is vertex 1: put it well away from the first
        v = [p, p + (0.7, 0.3, -0.4), p + (0.0, 0.3 * size, size), p, p + (0.0, 0.3 * size, size), p + (0.7, 0.36, -0.4)]
    return np.array(v)


PHASE = 0.8  # the lattice's turn about z, chosen so that no shadow is hidden in all six views (sole_shadows)


def lattice(n):
    """n near-uniform unit directions (Fibonacci sphere) and a radius in [1, 3] for each"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0)) + PHASE
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], 1), 1.0 + 2.0 * ((k * 0.7548776662) % 1.0)


def small_triangles(p, dirs, rad, ang=0.09):
    """one triangle per direction, square to it, circumradius ang * rad, turned by an angle of its own"""
    out = []
    for k, (d, r) in enumerate(zip(dirs, rad)):
        u = np.cross(d, (0.0, 0.0, 1.0) if abs(d[2]) < 0.9 else (1.0, 0.0, 0.0))
        u /= np.linalg.norm(u)
        v = np.cross(d, u)
        t = [2.0 * np.pi * j / 3.0 + 0.7 * k for j in range(3)]
        out.append([p + r * d + ang * r * (np.cos(a) * u + np.sin(a) * v) for a in t])
    return np.array(out).reshape(-1, 3, 3)


def small_spheres(p, dirs, rad, ang=0.06):
    return np.concatenate([p + rad[:, None] * dirs, (ang * rad)[:, None]], 1).reshape(-1, 4)


def occluders(p, n_tri, n_sph):
    """n_tri triangles and n_sph spheres sharing ONE lattice, kinds interleaved: each kind alone still
    surrounds P"""
    dirs, rad = lattice(n_tri + n_sph)
    is_tri = np.zeros(n_tri + n_sph, bool)
    if n_tri and n_sph:
        step = (n_tri + n_sph) / n_tri
        is_tri[np.unique((np.arange(n_tri) * step).astype(int))] = True
        assert is_tri.sum() == n_tri
    else:
        is_tri[:] = n_tri > 0
    return small_triangles(p, dirs[is_tri], rad[is_tri]), small_spheres(p, dirs[~is_tri], rad[~is_tri])


def views(c):
    """(eye, look) of the six cameras: 0.35 in front of the wall on +x, -x, +y, -y, +z, -z and 2 off its
    middle, looking at the opposite wall, which fills the frame.  Off the middle, because seen from a
    wall's middle an occluder on the axis hides its own shadow on the wall behind it; the look point is
    a little off too (default vup is +y, and nothing should be symmetric)."""
    c = np.asarray(c, float)
    out = []
    for m in range(3):
        for s in (1.0, -1.0):
            a, b = (m + 1) % 3, (m + 2) % 3
            eye, look = np.zeros(3), np.zeros(3)
            eye[m], eye[a], eye[b] = s * (HALF - 0.35), 1.6, -1.2
            look[m], look[a], look[b] = -s * HALF, 0.4 if m == 1 else 0.05, 0.0
            out.append((tuple(float(x) for x in (eye + c).astype(F32)), tuple(float(x) for x in (look + c).astype(F32))))
    return out


# ---- cases --------------------------------------------------------------------------------------------
def make_case(centre=(0.0, 0.0, 0.0), n_tri=0, n_sph=0, lights=None, tris=None, spheres=None, extra_tris=None,
              extra_spheres=None, which_views=range(6), light_faces=1):
    """a case is a dict of plain arrays; build() turns it into the scene dict.  `extra_*`: the primitives
    the case is about, kept apart from the lattice so that their effect can be shown by leaving them out"""
    c = np.asarray(centre, float)
    p = (c + P_OFF).astype(F32).astype(float)  # the light's vertex 0 as fp32 stores it
    lt, ls = occluders(p, n_tri, n_sph)
    case = {"centre": c, "p": p, "lights": [p] if lights is None else [np.asarray(q, float) for q in lights],
            "light_faces": light_faces,
            "tris": lt if tris is None else np.asarray(tris, float).reshape(-1, 3, 3),
            "spheres": ls if spheres is None else np.asarray(spheres, float).reshape(-1, 4),
            "extra_tris": np.zeros((0, 3, 3)) if extra_tris is None else np.asarray(extra_tris, float).reshape(-1, 3, 3),
            "extra_spheres": np.zeros((0, 4)) if extra_spheres is None else np.asarray(extra_spheres, float).reshape(-1, 4),
            "views": [views(c)[i] for i in which_views]}
    return case


def towards(p, tris):
    """the triangles wound so that cross(v1 - v0, v2 - v0) points to p's side: scan_row shades a surface
    only where dot(N, L) > 0, with the normal of the winding whichever side is looked at"""
    t = np.array(tris, float).reshape(-1, 3, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flip = ((p - t[:, 0]) * n).sum(axis=1) < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


def build(case, drop=None, extras=True):
    """case -> scene dict.  drop = ("tri" | "sph", k) leaves lattice occluder k out; extras=False leaves
    the case's own primitives out.  Geometry order: walls, lights, the case's own triangles, the lattice
    triangles; spheres: the case's own, then the lattice."""
    geoms = room_walls(case["centre"])
    for q in case["lights"]:
        v = light_triangles(q, case["light_faces"])
        geoms.append({"vertex": v.astype(F32), "face_index": np.arange(len(v)).reshape(-1, 3), "material": ol.LIGHT_A})
    tris, sph = case["tris"], case["spheres"]
    tint = 0.4 + 0.005 * (np.arange(len(sph)) % 100)  # a sphere keeps its colour when another is left out
    if drop is not None:
        kind, k = drop
        if kind == "tri":
            tris = np.delete(tris, k, axis=0)
        else:
            sph, tint = np.delete(sph, k, axis=0), np.delete(tint, k)
    tris = towards(case["p"], tris)
    xt = towards(case["p"], case["extra_tris"] if extras else case["extra_tris"][:0])
    xs = case["extra_spheres"] if extras else case["extra_spheres"][:0]
    for t, col in ((xt, (0.9, 0.6, 0.2)), (tris, (0.6, 0.6, 0.65))):
        if len(t):
            geoms.append({"vertex": t.reshape(-1, 3).astype(F32), "face_index": np.arange(3 * len(t)).reshape(-1, 3),
                          "material": _mat(col)})
    s = np.concatenate([xs, sph]).astype(F32)
    mats = np.stack([_mat((0.9, 0.6, 0.2))] * len(xs) + [_mat((t, 0.5, 0.8)) for t in tint]) \
        if len(s) else None
    return ol.scene_dict(geoms, s if len(s) else None, mats)


ROOMS = {"triangles": (96, 0), "spheres": (0, 96), "both kinds": (64, 64)}


@functools.lru_cache(maxsize=None)
def room(variant):
    n_tri, n_sph = ROOMS[variant]
    return make_case(n_tri=n_tri, n_sph=n_sph)


def _in_plane(p, n, h, ab):
    """points p + h n + a u + b v for (a, b) in ab; (u, v, n) orthonormal"""
    n = np.asarray(n, float) / np.linalg.norm(n)
    u = np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0))
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    return [p + h * n + a * u + b * v for a, b in ab]


def _fib(n):
    return lattice(n)[0]


def _case_cut_triangle():
    """one large triangle 1.2 from P, square to (1, 1, 1), corners 4 from its middle: it spans 146 degrees
    seen from P, lies across the faces +x, +y, +z and the cube corner between them"""
    c = make_case(n_tri=96)
    big = _in_plane(c["p"], (1, 1, 1), 1.2, [(4.0, 0.0), (-2.0, 3.4641), (-2.0, -3.4641)])
    # a second one towards (-1, -1, 0.3): across -x and -y, its plane 1.6 from P
    big2 = _in_plane(c["p"], (-1, -1, 0.3), 1.6, [(3.5, 0.2), (-2.0, 3.0), (-1.5, -3.2)])
    c["extra_tris"] = np.array([big, big2])
    return c


def _case_in_plane():
    """large triangles whose planes pass 1e-4, 1e-5, 1e-6 from P and through P itself: wall points and the
    triangles' own surfaces see P along those planes (cone entries of k_bin_light_tri_escape for those
    whose bounding ball does not hold P)"""
    c = make_case(n_tri=96)
    p = c["p"]
    y = float(F32(p[1] + 1e-4))
    z = float(F32(p[2] + 1e-6))
    t = [[(p[0] + 1.0, y, p[2] - 2.5), (p[0] + 4.5, y, p[2] - 2.0), (p[0] + 2.0, y, p[2] + 3.0)],
         [(p[0] - 4.0, p[1] - 3.0, z), (p[0] - 1.0, p[1] + 2.5, z), (p[0] - 1.2, p[1] - 3.5, z)],
         [(p[0], p[1] + 1.0, p[2] + 1.0), (p[0], p[1] + 4.0, p[2] + 1.5), (p[0], p[1] + 2.0, p[2] + 4.5)],
         _in_plane(p, (1, 1, 0), 1e-5, [(-3.5, -3.0), (-1.5, -3.5), (-2.5, -0.5)]),
         _in_plane(p, (0.3, -1, 0.5), 1e-4, [(1.0, 1.0), (3.5, 0.5), (2.0, 3.5)])]
    # P lies inside the bounding balls of those five: they are listed for every direction.  The same five
    # planes again with triangles of circumradius 1 whose middles are 3.4 from P: these leave cone entries
    for k, (n, h) in enumerate((((0, 1, 0), 1e-4), ((0, 0, 1), 1e-6), ((1, 0, 0), 0.0), ((1, 1, 0), 1e-5),
                                ((0.3, -1, 0.5), 1e-4))):
        phi = 0.9 + 1.3 * k
        m = 3.4 * np.array([np.cos(phi), np.sin(phi)])
        t.append(_in_plane(p, n, h, [m + (np.cos(phi + a), np.sin(phi + a)) for a in (0.3, 2.4, 4.5)]))
    c["extra_tris"] = np.array(t)
    return c


def _case_near_sphere():
    """a sphere whose surface is 0.01 from P, P outside: inside its reach, listed for every direction"""
    c = make_case(n_sph=96)
    d = np.array([0.6, 0.64, 0.48])
    c["extra_spheres"] = np.array([list(c["p"] + 0.31 * d) + [0.30]])
    return c


def _case_sphere_holds_p():
    """a sphere that contains P: every ray towards P from outside it ends in it; a second light outside
    lights the room, so the frame still tells one occluder from another"""
    c = make_case(n_sph=96, lights=None)
    c["lights"] = [c["p"], c["p"] + (2.0, 3.5, -1.0)]
    c["extra_spheres"] = np.array([list(c["p"] + (0.05, 0.03, -0.04)) + [0.12]])
    return c


def _case_near_triangle():
    """a small triangle 1e-3 from P: P inside its bounding ball, listed for every direction"""
    c = make_case(n_tri=96)
    c["extra_tris"] = np.array([_in_plane(c["p"], (0.5, 0.3, -0.8), 1e-3, [(0.05, 0.0), (-0.03, 0.045), (-0.025, -0.04)])])
    return c


def _case_cut_spheres():
    """spheres the plane x = P.x cuts.  The large one (1.5 away, radius 1.2) has a disc of 52 degrees that
    reaches to 30 degrees from the x axis: within the 54.74 degrees of the faces +x and -x, their short
    list.  The small ones (radius 0.1 at distance 2) stay 87 degrees from the axis: neither face lists
    them, the faces around do.  The same for the planes y = P.y and z = P.z."""
    c = make_case(n_sph=96)
    p = c["p"]
    c["extra_spheres"] = np.array([list(p + (0.2, 1.5, 0.1)) + [1.2],
                                   list(p + (0.02, -2.0, 0.3)) + [0.1],
                                   list(p + (-0.03, 0.4, 2.0)) + [0.1],
                                   list(p + (1.9, 0.05, -0.5)) + [0.1],
                                   list(p + (-1.4, -0.9, 0.02)) + [0.1],
                                   list(p + (-0.9, -0.1, -1.3)) + [0.95]])
    return c


def _line(p, d, n, r0, r1):
    d = np.asarray(d, float) / np.linalg.norm(d)
    return d, np.linspace(r0, r1, n)


def _case_cell_overflow(kind):
    """300 occluders behind one another on one line from P: more than kLightListCap (64) pair records in
    the cells of that direction"""
    c = make_case(n_tri=96 if kind == "tri" else 0, n_sph=96 if kind == "sph" else 0)
    d, r = _line(c["p"], (0.35, 0.25, 1.0), 300, 1.0, 4.4)
    dirs = np.tile(d, (300, 1))
    if kind == "tri":
        c["extra_tris"] = small_triangles(c["p"], dirs, r, ang=0.02)
    else:
        c["extra_spheres"] = small_spheres(c["p"], dirs, r, ang=0.015)
    return c


def _case_global_overflow(kind):
    """200 primitives P is within reach of: more than kTileGlobalCap (64) pair records on every face's short
    list.  Spheres of radius 0.0005 at 0.015 from P (the reach adds 0x1.6p-10 times the room's size, 0.02);
    needle triangles of length 0.02 and width 0.0002 whose middles are 0.005 from P (P inside the bounding
    ball).  Together they hide a few per cent of the directions."""
    c = make_case(n_tri=96 if kind == "tri" else 0, n_sph=96 if kind == "sph" else 0)
    dirs = _fib(200)
    if kind == "sph":
        c["extra_spheres"] = np.concatenate([c["p"] + 0.015 * dirs, np.full((200, 1), 0.0005)], 1)
    else:
        t = []
        for k, d in enumerate(dirs):
            a, b = _in_plane(np.zeros(3), d, 0.0, [(1.0, 0.0), (0.0, 1.0)])
            m = c["p"] + 0.005 * d
            t.append([m - 0.01 * a, m + 0.01 * a, m + 0.0002 * b])
        c["extra_tris"] = np.array(t)
    return c


def _case_lights(n):
    """two lights on opposite sides of the occluders (the second below them), or five spread over the
    room (the fifth gets no lists): quirk S3 hands the first occluder's t2 on to the next light"""
    c = make_case(n_tri=64, n_sph=64)
    p = c["p"]
    c["lights"] = [p + (0.2, 4.0, -0.3), p + (-0.3, -4.1, 0.4)] if n == 2 else \
        [p, p + (3.5, 3.0, -2.5), p + (-3.8, -3.2, 1.0), p + (1.0, -2.0, 4.2), p + (-2.0, 4.2, -3.9)]
    return c


def _case_far():
    """the room 2,000 units from the world origin: the `delta` term of the reach"""
    return make_case(centre=(1300.0, -1000.0, 1150.0), n_tri=64, n_sph=64)


def _case_two_shells():
    """the lattice twice along the SAME 64 directions, at radius 1.4 to 1.6 and at twice that, both kinds,
    each occluder with the angular size and turn of its twin: seen from P an outer occluder fills the
    directions its inner twin fills, so nearly every ray that needs it is occluded by the twin as well and
    no frame shows whether the outer one was listed"""
    c = make_case()
    dirs, rad = lattice(64)
    rad = 1.4 + 0.1 * (rad - 1.0)
    is_tri = np.arange(64) % 2 == 0
    c["tris"] = np.concatenate([small_triangles(c["p"], dirs[is_tri], k * rad[is_tri]) for k in (1.0, 2.0)])
    c["spheres"] = np.concatenate([small_spheres(c["p"], dirs[~is_tri], k * rad[~is_tri]) for k in (1.0, 2.0)])
    c["shell"] = 32  # occluders per shell and kind: the first 32 of each kind are the inner shell
    return c


WALL_GAP = 0.05
WALL_ANG = 0.012
WALL_SPAN = 0.6  # the lattice spheres are 1 to 1 + WALL_SPAN from P


def _case_beside_wall():
    """P 0.05 from the wall on -x, small spheres (angular radius 0.012) on the lattice around it -- those of
    384 directions that lie inside the room.  The box reach R0 of such a sphere is mostly the 0x1.6p-10 W term
    (W: to the far corner of the room, 12 and more); the cone of origins through it ends at a wall a few units
    on, so the rectangles' reach Rx of k_bin_light_pairs is well below R0.  The face -x sees 0.1 x 0.1 of the
    wall beside P and nothing else: a seventh camera 0.3 from the wall looks at that patch, and one sphere of the
    case's own sits between P and the wall and shadows the middle of it (P is within its reach: listed for
    every direction)."""
    c = make_case()
    p = np.array([-HALF + WALL_GAP, P_OFF[1], P_OFF[2]]).astype(F32).astype(float)
    dirs, rad = lattice(384)
    s = small_spheres(p, dirs, 1.0 + WALL_SPAN * (rad - 1.0) / 2.0, ang=WALL_ANG)
    inside = (np.abs(s[:, :3]) + s[:, 3:] < HALF - 0.01).all(axis=1)
    c["p"], c["lights"], c["spheres"] = p, [p], s[inside]
    c["extra_spheres"] = np.array([list(p + (-0.025, 0.003, -0.002)) + [0.0143]])
    foot = (-HALF, p[1], p[2])
    c["views"] = c["views"] + [(tuple(float(x) for x in np.array([-HALF + 0.3, p[1] + 0.11, p[2] - 0.07], F32)),
                                tuple(float(x) for x in np.array(foot, F32)))]
    return c


CASES = {
    "triangle cut by face planes": _case_cut_triangle,
    "P nearly in triangles' planes": _case_in_plane,
    "P inside a sphere's reach": _case_near_sphere,
    "P inside a sphere": _case_sphere_holds_p,
    "P beside a small triangle": _case_near_triangle,
    "spheres cut by face planes": _case_cut_spheres,
    "cell overflow, spheres": lambda: _case_cell_overflow("sph"),
    "cell overflow, triangles": lambda: _case_cell_overflow("tri"),
    "global overflow, spheres": lambda: _case_global_overflow("sph"),
    "global overflow, triangles": lambda: _case_global_overflow("tri"),
    "spheres grouped, triangles not": lambda: make_case(n_tri=20, n_sph=96),
    "triangles grouped, spheres not": lambda: make_case(n_tri=96, n_sph=20),
    "two lights": lambda: _case_lights(2),
    "five lights": lambda: _case_lights(5),
    "far from the origin": _case_far,
    "two shells": _case_two_shells,
    "light beside a wall": _case_beside_wall,
}
# what the GPU test expects of the lists: the kinds that have them, and which count must exceed its cap
# "seen": the case's own primitives are large enough to show in a frame, so some pixels they change are lit;
# the others sit within 0.12 of P and change a pixel only by shadowing it
EXPECT = {name: {"sph": True, "tri": True, "over": None,
                 "seen": name not in ("P inside a sphere", "global overflow, spheres", "global overflow, triangles")}
          for name in CASES}
for _n in ("triangle cut by face planes", "P nearly in triangles' planes", "P beside a small triangle",
           "cell overflow, triangles", "global overflow, triangles", "triangles grouped, spheres not"):
    EXPECT[_n]["sph"] = False
for _n in ("P inside a sphere's reach", "P inside a sphere", "spheres cut by face planes", "cell overflow, spheres",
           "global overflow, spheres", "spheres grouped, triangles not", "light beside a wall"):
    EXPECT[_n]["tri"] = False
for _n in CASES:
    if "overflow" in _n:
        EXPECT[_n]["over"] = "cell" if _n.startswith("cell") else "global"


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def fixed_face_case():
    """a two-face light at the room's middle: ESC_FACE_FIXED face 0 samples vertex 0, face 1 vertex 1"""
    return make_case(n_tri=64, n_sph=64, light_faces=2)


# ---- the reference ------------------------------------------------------------------------------------
def light_points(d):
    """the sample points the product computes for the scene (host only): (n, 3) fp32"""
    return ol.scene_to_product(d).table("light_points").view(F32).reshape(-1, 4)[:, :3].copy()


def frame(d, view, size=None, **kw):
    w = h = size or W
    return ol.oracle_render(d, view[0], view[1], w, h, threads=8, **kw)


def lit_and_shadowed(d, view, **kw):
    """-> (hit, shadowed): pixels that show something, and those of them that some light does not reach
    (scan_row adds nothing for an occluded light, and at least ka / 2 for one that is not)"""
    on, off = frame(d, view, **kw), frame(d, view, shadows=False, **kw)
    return (off != 0).any(axis=2), (on.view(np.uint32) != off.view(np.uint32)).any(axis=2)


def camera_hits(d, view, size=None):
    """ray_oracle's closest hit of every camera ray -> (hit mask, hit points, geom, prim)"""
    from ray_cases import camera_targets
    w = h = size or W
    o, t = camera_targets(view[0], view[1], w, h)
    dirs = ro.normalize((t - o).astype(F32))
    hit, _ = ro.ref_queries(d, o, dirs)
    ok = hit["prim"] >= 0
    pts = (o + dirs * hit["t"][:, None]).astype(np.float64)
    return ok, pts, hit["geom"], hit["prim"]


def face_of(v):
    """the cube face of directions v (n, 3), as light_list_cell picks it: 2 * dominant axis + (negative)"""
    m = np.argmax(np.abs(v), axis=1)
    return 2 * m + (v[np.arange(len(v)), m] < 0)


def face_shares(d, case_views, p, size=None):
    """share of all shadow-ray origins (closest hits of the views' camera rays) per cube face around p"""
    n = np.zeros(6)
    per_view = []
    for v in case_views:
        ok, pts, _, _ = camera_hits(d, v, size)
        f = np.bincount(face_of(pts[ok] - p), minlength=6)
        per_view.append(f)
        n += f
    return n / n.sum(), per_view


def sole_shadows(c, size=None):
    """for every lattice occluder: the pixels, over the case's views, that change when it alone is left
    out and that do not show it (so the change is a shadow only it casts) -> {("tri" | "sph", k): count}"""
    d = build(c)
    n_geom = len(d["geometry"])
    tri_geom = n_geom - 1 if len(c["tris"]) else -1
    full, shows = [], []
    for v in c["views"]:
        full.append(frame(d, v, size))
        ok, _, geom, prim = camera_hits(d, v, size)
        shows.append((ok, geom, prim))
    out = {}
    for kind, n in (("tri", len(c["tris"])), ("sph", len(c["spheres"]))):
        for k in range(n):
            dk = build(c, drop=(kind, k))
            cnt = 0
            for v, f, (ok, geom, prim) in zip(c["views"], full, shows):
                mine = ok & ((prim == k) & (geom == tri_geom) if kind == "tri" else (prim == k + len(c["extra_spheres"])) & (geom < 0))
                diff = (frame(dk, v, size).view(np.uint32) != f.view(np.uint32)).any(axis=2).reshape(-1)
                cnt += int((diff & ~mine).sum())
            out[(kind, k)] = cnt
    return out


def extras_matter(c, **kw):
    """per view: (pixels the case's own primitives change, those of them that are shadowed, those lit)"""
    d, d0 = build(c), build(c, extras=False)
    out = []
    for v in c["views"]:
        hit, sh = lit_and_shadowed(d, v, **kw)
        m = (frame(d, v, **kw).view(np.uint32) != frame(d0, v, **kw).view(np.uint32)).any(axis=2)
        out.append((int(m.sum()), int((m & hit & sh).sum()), int((m & hit & ~sh).sum())))
    return out


# ---- scenes of their own: a floor under a one-point light, spheres in between ----------------------------------
def slab_scene(spheres, light=(0.3, 10.0, -0.2), floor_y=-1.5, half=12.0):
    p = np.asarray(light, np.float32).astype(float)
    q = np.array([(-half, floor_y, -half), (half, floor_y, -half), (half, floor_y, half), (-half, floor_y, half)])
    floor = towards(p, q[[0, 1, 2, 0, 2, 3]])
    grey = ol.material13(ka=(0.6, 0.6, 0.65), kd=(0.6, 0.6, 0.65))
    geoms = [{"vertex": floor.reshape(-1, 3).astype(np.float32), "face_index": np.arange(6).reshape(2, 3), "material": grey},
             {"vertex": light_triangles(p).astype(np.float32), "face_index": np.arange(3).reshape(1, 3),
              "material": ol.LIGHT_A}]
    s = np.asarray(spheres, np.float32)
    mats = np.stack([ol.material13(ka=(0.4 + 0.005 * (k % 100), 0.5, 0.8), kd=(0.4 + 0.005 * (k % 100), 0.5, 0.8))
                     for k in range(len(s))])
    return ol.scene_dict(geoms, s, mats)


SLAB_VIEWS = [((0.5, 3.0, 7.0), (0.0, -1.5, 0.0)), ((-6.0, 2.5, -3.0), (1.0, -1.5, 1.0))]


@functools.lru_cache(maxsize=None)
def far_apart_scene():
    """80 spheres of radius 0.02 spread thinly over a slab 16 wide, 10 below the light: a k-d leaf of 8
    spans several units, i.e. tens of cells seen from P"""
    rng = np.random.default_rng(12)
    n = 80
    s = np.stack([rng.uniform(-8, 8, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-8, 8, n), np.full(n, 0.02)], 1)
    return slab_scene(s)


@functools.lru_cache(maxsize=None)
def overlapping_scene():
    """64 clusters of two spheres 0.01 apart (original indices 2 k, 2 k + 1) on a jittered 8 x 8 grid of
    spacing 2: the splits of the k-d order fall between clusters, a leaf's spheres are in index order, so
    most records hold the two spheres of one cluster -- and seen from P they fill the same cells"""
    rng = np.random.default_rng(5)
    s = []
    for k in range(64):
        x, z = 2.0 * (k % 8) - 7.0 + rng.uniform(-0.3, 0.3), 2.0 * (k // 8) - 7.0 + rng.uniform(-0.3, 0.3)
        s += [(x, 0.0, z, 0.15), (x + 0.01, 0.0, z, 0.15)]
    return slab_scene(np.array(s))


def corner_case(lights):
    """the room's lattice, a light in a corner of the scene box, a sphere so close to it that its reach
    exceeds half its distance, and one in the direction of the box's far edge"""
    c = make_case(n_sph=96)
    corner = np.array([4.5, 4.4, 4.6], np.float32).astype(float)
    c["lights"] = [corner if q == "corner" else c["p"] for q in lights]
    c["extra_spheres"] = np.array([list(corner + 0.1 * np.array([-0.6, -0.64, -0.48])) + [0.035],
                                   list(corner + 0.3 * np.array([-11.0, -10.9, -0.1])) + [0.15]])
    return c, corner


CORNER_ORDERS = [("corner",), ("centre", "corner"), ("corner", "centre")]


# ---- the shadow rays the reference traces, and what each of them needs -----------------------------------------
# A shadow ray of the frame tests the pair records of ONE cell of its light's cube map plus that face's short
# list (rt_lists.h "Light lists").  A record missing from the cell changes a pixel only where the dropped
# primitive is the ray's only occluder (the last light) or its first one in index order (an earlier light,
# through quirk S3).  `needed` does not care: every primitive the reference's any-hit test accepts for the
# ray with the ray's own initial t counts, whether or not another one would have ended the sweep before it.
BORDER = 2.0 ** -12  # cells: a ray this close to a cell border is held to both cells (cell_of)


def primary_rays(view, size=None):
    """the reference's primary rays of a view: (origin (3,), dirs (size * size, 3)) fp32, ray h * size + w.
    camera.h:16-34 through the oracle's own camera (orc_camera_init), get_ray restated one rounding per step"""
    n = size or W
    cam = ol.oracle_camera(view[0], view[1], n, n)
    o, llc, hor, ver = (np.array(list(x), F32) for x in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical))
    s = (np.arange(n, dtype=F32) / F32(n - 1)).astype(F32)
    a = (llc[None, None, :] + (hor[None, None, :] * s[None, :, None]).astype(F32)).astype(F32)
    a = (a + (ver[None, None, :] * s[:, None, None]).astype(F32)).astype(F32)
    a = (a - o).astype(F32).reshape(-1, 3)
    return o, ro.normalize(a)


def triangles_of(d):
    """(n, 3, 3) fp32: the scene's triangles by original index (faces geometry by geometry)"""
    return np.concatenate([g["vertex"][g["face_index"].astype(int)] for g in d["geometry"]]).astype(F32)


def accepts(d, o, dirs, tb):
    """the reference's any-hit tests of rays (o, dirs) with initial t = tb against every primitive
    -> {"tri": [n_rays, n_tri] bool, "sph": [n_rays, n_sph] bool}, (first acceptor in the reference's order
    (triangles, then spheres; -1: none), its t2)"""
    tris, sph = triangles_of(d), d["spheres"]
    n = len(o)
    acc = {"tri": np.zeros((n, len(tris)), bool), "sph": np.zeros((n, len(sph)), bool)}
    first = np.full(n, -1, int)
    t_first = np.zeros(n, F32)
    for i, tv in enumerate(tris):
        ok, t2, _, _ = ro.tri_test(o, dirs, tv[0], tv[1], tv[2])
        a = ok & ~(t2 >= tb)
        acc["tri"][:, i] = a
        new = a & (first < 0)
        first[new], t_first[new] = i, t2[new]
    for i, s in enumerate(sph):
        ok, t2 = ro.sph_test(o, dirs, s)
        a = ok & ~(t2 >= tb)
        acc["sph"][:, i] = a
        new = a & (first < 0)
        first[new], t_first[new] = len(tris) + i, t2[new]
    return acc, first, t_first


def shadow_rays(d, view, size=None, fixed_face=0):
    """the shadow rays scan_row traces for a view (oracle/rt_oracle.c scan_row, main.cpp:740-772), for every
    pixel that hits and every light, in the reference's order (pixel h * size + w, then light):
        hitp = origin + dir * (t_use - eps);  L = normalize(P - hitp);  tb = length(P - hitp) - eps
    every step rounded to fp32, P = vertex[fixed_face] + 0 of the light's geometry (quirk S2) and t_use what the
    light before left in t (quirk S3): the t2 of the first accepting primitive in index order, otherwise its
    len - eps; the camera's closest t for the first light.
    -> dict of arrays over the rays: "pixel", "light", "hitp", "L", "tb", "occluded", "facing" (dot(N, L) > 0:
    an unoccluded light adds to the pixel), and "P" (n_lights, 3), "n_pixels", "origin", "dirs" """
    o, dirs = primary_rays(view, size)
    oo = np.broadcast_to(o, dirs.shape)
    hit, _ = ro.ref_queries(d, oo, dirs)
    ok = hit["prim"] >= 0
    pix = np.flatnonzero(ok)
    hk = {k: v[ok] for k, v in hit.items()}
    dr = dirs[ok]
    N, _, has = ro.normals_and_ks(d, hk, np.ascontiguousarray(oo[ok]), dr)
    assert has.all()
    lights = d["light_sources"]
    P = np.array([(d["geometry"][g]["vertex"][fixed_face] + F32(0)).astype(F32) for g in lights], F32).reshape(-1, 3)
    t = hk["t"].copy()
    cols = {k: [] for k in ("hitp", "L", "tb", "occluded", "facing")}
    with np.errstate(all="ignore"):
        for li in range(len(lights)):
            hitp = (o + (dr * (t - ro.EPS).astype(F32)[:, None]).astype(F32)).astype(F32)
            L = (P[li] - hitp).astype(F32)
            ln = np.sqrt(ro.dot(L, L)).astype(F32)
            tb = (ln - ro.EPS).astype(F32)
            L = (L / ln[:, None]).astype(F32)
            _, first, t_first = accepts(d, hitp, L, tb)
            occ = first >= 0
            t = np.where(occ, t_first, tb).astype(F32)
            for k, v in (("hitp", hitp), ("L", L), ("tb", tb), ("occluded", occ), ("facing", ro.dot(N, L) > 0)):
                cols[k].append(v)
    nl = len(lights)
    out = {k: np.stack(v, axis=1).reshape((len(pix) * nl,) + v[0].shape[1:]) for k, v in cols.items()}
    out["pixel"] = np.repeat(pix, nl)
    out["light"] = np.tile(np.arange(nl), len(pix))
    out.update(P=P, n_pixels=len(dirs), origin=o, dirs=dirs)
    return out


def implied_split(rays):
    """per pixel, from the restated rays alone -> (hit, sure, maybe): `sure`: the frame with shadows MUST differ
    from the one without (the first occluded light of the pixel faces the surface: without shadows it adds at
    least ka / 2 / n_lights, with them nothing, and up to that light both frames took the same steps);
    `maybe`: some light is occluded.  A frame differs only where `maybe` holds (no occluded light: the same
    steps throughout).  Between the two lie the pixels whose first occluded light faces away: what it hands on
    through quirk S3 may or may not change a later light's share; with one light there are none that change."""
    nl = len(rays["P"])
    occ = rays["occluded"].reshape(-1, nl)
    fac = rays["facing"].reshape(-1, nl)
    pix = rays["pixel"].reshape(-1, nl)[:, 0]
    k = np.argmax(occ, axis=1)  # the first occluded light, where there is one
    any_occ = occ.any(axis=1)
    first_faces = any_occ & fac[np.arange(len(k)), k]
    hit, sure, maybe = (np.zeros(rays["n_pixels"], bool) for _ in range(3))
    hit[pix] = True
    sure[pix], maybe[pix] = first_faces, any_occ
    if nl == 1:
        maybe = sure.copy()  # an occluded light that faces away adds nothing either way, and nobody comes after it
    return hit, sure, maybe


def needed(d, rays):
    """per ray the original primitives whose reference any-hit test accepts it -- ro.tri_test / ro.sph_test and
    ~(t2 >= tb) with the ray's own initial tb -> {"tri": [n_rays, n_tri] bool, "sph": [n_rays, n_sph] bool}"""
    with np.errstate(all="ignore"):
        return accepts(d, rays["hitp"], rays["L"], rays["tb"])[0]


def face_axes(face):
    """(m, ia, ib, sign) of light_face_axes / light_list_cell: the face's axis, the axes of u and w"""
    m = face >> 1
    return m, (1 if m == 0 else 0), (1 if m == 2 else 2), (-1.0 if face & 1 else 1.0)


def cell_of(P, hitp, R):
    """light_list_cell (rt_lists.h) restated for rays that start at hitp (n, 3) towards P: v = hitp - P in fp32;
    the dominant axis exactly as the kernel picks it (strict >, order x, y, z) and the face 2 m + (negative);
    the coordinates (va / dm + 1) R / 2 in float64.  The kernel divides with v_rcp_f32 (3e-5 cells, it says), so
    its cell cannot be had bit for bit: a coordinate within BORDER = 2^-12 cells of a cell border stands for
    both cells -- both binning kernels grow their extents by 1e-3 cells, and 2^-12 + 3e-5 < 1e-3.
    -> (face (n,), cells (n, 4): index (face R + cw) R + cu within the light, repeated where there is one,
    u (n,), w (n,))"""
    v = (np.asarray(hitp, F32) - np.asarray(P, F32)).astype(F32)
    a = np.abs(v)
    n = len(v)
    m = np.zeros(n, int)
    dm = a[:, 0].copy()
    for k in (1, 2):
        g = a[:, k] > dm
        m[g], dm[g] = k, a[g, k]
    vm = v[np.arange(n), m]
    va = np.where(m == 0, v[:, 1], v[:, 0]).astype(np.float64)
    vb = np.where(m == 2, v[:, 1], v[:, 2]).astype(np.float64)
    face = 2 * m + (vm < 0)
    with np.errstate(all="ignore"):
        u = np.nan_to_num((va / dm.astype(np.float64) + 1.0) * (R / 2.0))
        w = np.nan_to_num((vb / dm.astype(np.float64) + 1.0) * (R / 2.0))

    def both(x):
        return [np.clip(np.floor(x + s), 0, R - 1).astype(int) for s in (-BORDER, BORDER)]
    cells = np.stack([(face * R + cw) * R + cu for cw in both(w) for cu in both(u)], axis=1)
    return face, cells, u, w


def in_box(header, hitp):
    """shadow_wave_lists' test (rt_kernels.hip): the lists serve a ray only if its origin lies in the grown
    scene box, fp32 compares against scene_lo / scene_hi = header[4:7] / header[7:10]"""
    lo, hi = np.asarray(header[4:7], F32), np.asarray(header[7:10], F32)
    h = np.asarray(hitp, F32)
    return ((h >= lo) & (h <= hi)).all(axis=1)


def sphere_reaches(header, P, centre, r2):
    """(R0, Rx) of k_bin_light_pairs for one sphere (centre, r2 as the sorted record holds them) and sample
    point P, in float64 from rt_lists.h's formulas: the box reach and the reach from the cone of origins"""
    hdr = np.asarray(header, np.float64)
    g, rho, lo, hi = hdr[0:3], hdr[3], hdr[4:7], hdr[7:10]
    P, C = np.asarray(P, np.float64), np.asarray(centre, np.float64)
    k = float.fromhex("0x1.6p-10")
    delta = 2.0 ** -20 * (rho + np.abs(P - g).sum())
    far = np.sqrt((np.maximum(np.abs(C - lo), np.abs(C - hi)) ** 2).sum())
    rad = np.sqrt(max(0.0, float(r2)))
    R0 = (rad + k * far) * (1.0 + 2.0 ** -20) + delta + 2.0 ** -60
    c = C - P
    cn = np.sqrt(c @ c)
    Rx = R0
    if ((P >= lo) & (P <= hi)).all() and R0 <= 0.5 * cn:
        phi0 = np.arcsin(R0 / cn) * (1.0 + 1e-9) + 1e-12
        s_max = np.inf
        for a in range(3):
            e = c[a] / cn
            room_ = abs(e) * (1.0 - 1e-9) - phi0
            if room_ > 0.0:
                s_max = min(s_max, ((hi[a] - P[a] if e > 0.0 else P[a] - lo[a]) + delta) / room_)
        if np.isfinite(s_max):
            W1 = (max(cn, s_max - cn) + s_max * phi0) * (1.0 + 1e-9) + delta
            Rx = (rad + k * min(far, W1)) * (1.0 + 2.0 ** -20) + delta + 2.0 ** -60
    return R0, Rx


_members = {}


def members(key, d, view, fixed_face=0):
    """shadow_rays and needed of one (scene, view), computed once per `key` and left unchanged"""
    if key not in _members:
        rays = shadow_rays(d, view, fixed_face=fixed_face)
        nd = needed(d, rays)
        for a in list(rays.values()) + list(nd.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _members[key] = (rays, nd)
    return _members[key]


def membership_figures(key, d, views, fixed_face=0, R=128, li=0):
    """what light li's rays of all the views need, cell by cell (a ray on a border: its lower cell), cached rays:
      "origins" [6] cells per face that hold a ray origin, "needing" [6] those of them where some ray needs
      something, "pairs" the distinct needed (cell, kind, primitive) triples, "hidden" those of them reached ONLY
      by rays that a second primitive accepts as well -- no frame comparison can notice them missing --, "rays"
      the number of rays of all lights, "inside" [n_lights] the share of each light's rays that start in the scene
      box (in_box against the scene's header table)"""
    hdr = ol.scene_to_product(d).table("header").view(F32)
    origins, needing = [set() for _ in range(6)], [set() for _ in range(6)]
    every, sole = set(), set()
    n_rays, nl = 0, len(d["light_sources"])
    inside, total = np.zeros(nl), np.zeros(nl)
    for vi, view in enumerate(views):
        rays, nd = members((key, vi, fixed_face), d, view, fixed_face)
        n_rays += len(rays["tb"])
        box = in_box(hdr, rays["hitp"])
        inside += np.bincount(rays["light"], weights=box, minlength=nl)
        total += np.bincount(rays["light"], minlength=nl)
        m = rays["light"] == li
        face, cells, _, _ = cell_of(rays["P"][li], rays["hitp"][m], R)
        cell = cells[:, 0]
        n_acc = nd["tri"][m].sum(axis=1) + nd["sph"][m].sum(axis=1)
        for f in range(6):
            origins[f].update(cell[face == f].tolist())
            needing[f].update(cell[(face == f) & (n_acc > 0)].tolist())
        for kind in ("tri", "sph"):
            r, q = np.nonzero(nd[kind][m])
            every.update(zip(cell[r].tolist(), [kind] * len(r), q.tolist()))
            alone = n_acc[r] == 1
            sole.update(zip(cell[r[alone]].tolist(), [kind] * int(alone.sum()), q[alone].tolist()))
    return {"origins": [len(s) for s in origins], "needing": [len(s) for s in needing], "pairs": every,
            "hidden": every - sole, "rays": n_rays, "inside": inside / np.maximum(total, 1)}
