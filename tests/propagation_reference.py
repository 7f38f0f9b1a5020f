"""Float64 numpy statements of what the propagation kernels assemble from their pieces -- the first DOM on a ray and the absorption
lengths used up on a straight segment -- together with the independent single-function formulas they are made of.  Nothing here
shares code or expression order with oracle/ or clsim_amd/csrc/: the DOM search is brute force over the geometry dict (no cells,
no string sets, no z layers, no string_max_radius), the layer walk integrates over the layer grid of the medium dict.
tests/test_propagation_reference.py holds the oracle to these statements, tests/test_propagation_reference_gpu.py the kernels.

THE ROUNDING MODEL BEHIND THE TOLERANCES.  u = 2^-24 is the unit roundoff of binary32 (one rounding to nearest changes a value v by
at most u |v|); ulp(v) = 2 u |v| at most.  The statements take the kernels' float32 INPUTS (step position, theta, phi, time, weight,
recorded positions) as exact and compute in float64, so every bound below counts the float32 roundings of the reference's own
expression (sparse_collision_kernel.c.cl, propagation_kernel.c.cl, restated in oracle/clsim_oracle.c), first order in u.

(1) The decision of the search: disc = urdot^2 - dr2 + R^2 with dx = c - p (three subtractions), dr2 = (dx^2 + dy^2) + dz^2, urdot =
    (dx dirx + dy diry) + dz dirz, r^2 = |c - p|^2.
      * The roundings of dx, dy, dz and of the direction's components move the DOM, or turn the ray, by u r resp. ~8 u r sideways:
        that changes the impact parameter rho, and disc = R^2 - rho^2 by 2 rho (delta rho) <= 2 R (9 u r) -- a GEOMETRIC term (below),
        because urdot^2 and dr2 change together.
      * What does not cancel are the roundings of the arithmetic at magnitude r^2: urdot's three products (together <= u r by
        Cauchy-Schwarz) and two sums (2 u r) give (delta urdot) <= 3 u r, so urdot^2 moves by 6 u r^2; squaring it 1 u r^2; dr2's three
        squares together 1 u r^2 and its two sums 2 u r^2; the final subtraction and the addition of R^2 round a small number.
      => k = 6 + 1 + 1 + 2 = 10, E_round = K_DISC u max(r^2, 1).  (A probe with k = 8 had explained every disagreement it saw.)
      * The geometric term also holds the reference's own DOM positions: GeometrySource.cxx:499-709 stores x and y as 16 bit
        multiples of max|x - string mean| / 32767 (truncated: up to one quantum per axis), shares a position template between
        strings whose DOMs agree within 1e-4 m per axis, and z and the string means are float literals (u |coordinate|).  dom_position
        _error() adds these up from the geometry dict: delta_c.
      => E(r) = K_DISC u max(r^2, 1) + 2 R (delta_c + 9 u r).
    At r = 750 m: E = 0.34 m^2 against R^2 = 0.68 m^2 -- the reference's search decides impact parameters to E / (2 R) ~ +-0.2 m there
    (k = 8: +-0.16 m), and beyond ~1070 m E > R^2: no ray is decided.
(2) The distance: s = urdot - sqrt(disc) / pancake.  d sqrt(disc) = E / (2 sqrt(disc)); urdot itself 3 u r + the geometric delta_c +
    9 u r; the subtraction u s.  => delta_s = E / (2 pancake sqrt(disc)) + delta_c + 14 u r.
(3) The record: position = p + s dir - c' in float32 at coordinates of magnitude M = max |coordinate| : three roundings each,
    delta_pos = delta_s + delta_c + 4 ulp(M).  t = st + s / v: delta_t = delta_s / v + 2 ulp(t).  theta = acos(dirz), phi = atan2:
    oracle_math's acos and atan2 are good to ~2 ulp, the direction to ~4 u per component, and acos amplifies an error of its
    argument by 1 / sin(theta): delta_theta = u (8 + 8 / |sin theta|) + 2 ulp(pi), delta_phi = 8 u / |sin theta| + 2 ulp(2 pi).
    weight = w / bias: weight_bound(), with the table's slope.  groupVelocity: 8 u relative (a degree four polynomial
    twice, a product, a division).
(4) The walk (absorption_lengths_used): see its docstring.
(5) The bounds (2) ... (4) are FIRST ORDER worst cases with every operation rounded correctly.  The reference's math functions are not
    (log, sincos, acos, atan2, powr, exp: up to ~2.5 ulp, tests/test_oracle.py), literals carry their own rounding, and the second
    order is left out.  The tests therefore assert SAFETY = 4 times the first order bound -- and hold the ORACLE, on the CPU, to the
    first order bound itself (a quarter of what is asserted: the factor of four of head-room).  Which rays rounding DECIDES is
    judged with E as it stands, never with a multiple.

Reference behaviour that the statements spell out as CLASSES of rays (they are counted by the tests, not hidden in a tolerance):
  * vertical: dirx^2 + diry^2 == 0 -- the reference never searches (sparse_collision_kernel.c.cl:511-512); never detected.
  * start inside: entry distance s < 0 <= exit distance for some DOM -- not detected ON THAT DOM (c.cl:150-159: smin1 < 0), the ray
    goes on to the next one.  With a pancake factor the ellipsoid is the one flattened along the ray.
  * fragile: decided by rounding, first_dom() below.
"""
import math

import numpy as np

U = 2.0 ** -24
K_DISC = 10.0                    # (1) above
SAFETY = 4.0                     # (5) above
C_LIGHT = 0.299792458            # m / ns
NM = 1e-9


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# single functions (double precision, from the reference's HOST classes)
# ---------------------------------------------------------------------------------------------------------------------------------

def tilt_independent(medium, pos):
    """the tilt in double precision numpy, stated from ScalarFieldIceTiltZShift.cxx:145-213: bilinear between the dust-logger
    profiles along the tilt direction and in z, the outermost cells extended linearly beyond the table"""
    tl = medium["tilt"]
    d = np.asarray(tl["distances"], dtype=np.float64)
    zc = np.asarray(tl["zcoords"], dtype=np.float64)
    corr = np.asarray(tl["zcorr"], dtype=np.float64).reshape(len(d), len(zc))
    p = pos.astype(np.float64)
    zr = (p[:, 2] - zc[0]) / ((zc[-1] - zc[0]) / (len(zc) - 1))
    k = np.clip(np.floor(zr).astype(int), 0, len(zc) - 2)
    fz = zr - k
    nr = math.cos(tl["azimuth"]) * p[:, 0] + math.sin(tl["azimuth"]) * p[:, 1]
    j = np.clip(np.searchsorted(d, nr, side="right"), 1, len(d) - 1)
    lower = corr[j - 1, k + 1] * fz + corr[j - 1, k] * (1 - fz)
    upper = corr[j, k + 1] * fz + corr[j, k] * (1 - fz)
    f_lower = (d[j] - nr) / (d[j] - d[j - 1])
    return upper * (1 - f_lower) + lower * f_lower


def ppc_anisotropy(dirs, azimuth, k1, k2):
    """the formula resources/tests/testScalarFields.py:52-91 tests the device against (its Python port of PPC), vectorised"""
    azx, azy = math.cos(azimuth), math.sin(azimuth)
    k1e, k2e = math.exp(k1), math.exp(k2)
    kz = 1.0 / (k1e * k2e)
    n = dirs.astype(np.float64)
    s1 = (azx * n[:, 0] + azy * n[:, 1]) ** 2
    s2 = (-azy * n[:, 0] + azx * n[:, 1]) ** 2
    s3 = n[:, 2] ** 2
    l1, l2, l3 = k1e * k1e, k2e * k2e, kz * kz
    B2 = 1.0 / l1 + 1.0 / l2 + 1.0 / l3
    nB = s1 / l1 + s2 / l2 + s3 / l3
    An = s1 * l1 + s2 * l2 + s3 * l3
    return 1.0 / ((B2 - nB) * An / 2.0)


def icecube_absorption_length(m, layer, wlen):
    """AbsLenIceCube.cxx:63-67 (GetValue), wavelengths in metres"""
    x = np.asarray(wlen, dtype=np.float64) / NM
    return 1.0 / ((m["D"] * m["aDust400"][layer] + m["E"]) * x ** (-m["kappa"]) + m["A"] * np.exp(-m["B"] / x) * (1.0 + 0.01 * m["deltaTau"][layer]))


def icecube_scattering_length(m, layer, wlen):
    """ScatLenIceCube.cxx:54-58"""
    x = np.asarray(wlen, dtype=np.float64) / NM
    return 1.0 / (m["b400"][layer] * (x / 400.0) ** (-m["alpha"]))


def icecube_phase_index(n, wlen):
    """RefIndexIceCube.cxx:84-101"""
    xm = np.asarray(wlen, dtype=np.float64) / 1e-6
    return n[0] + xm * (n[1] + xm * (n[2] + xm * (n[3] + xm * n[4])))


def icecube_group_index(n, g, wlen):
    xm = np.asarray(wlen, dtype=np.float64) / 1e-6
    return icecube_phase_index(n, wlen) * (g[0] + xm * (g[1] + xm * (g[2] + xm * (g[3] + xm * g[4]))))


def table_value(tab, wlen):
    """FunctionFromTable.cxx:105-122, equal spacing: linear between the entries, the end values beyond them"""
    v = np.asarray(tab["values"], dtype=np.float64)
    grid = tab["start"] + tab["step"] * np.arange(len(v))
    return np.interp(np.asarray(wlen, dtype=np.float64), grid, v)


def group_velocity(medium, wlen):
    """c / n_group: the IceCube polynomials or the medium's table (MediumPropertiesSource.cxx:255-272)"""
    if "group_table" in medium:
        return C_LIGHT / table_value(medium["group_table"], wlen)
    return C_LIGHT / icecube_group_index(medium["n"], medium["g"], wlen)


def wavelength_bias(bias, wlen):
    return table_value(bias, wlen) if bias["kind"] == "table" else np.full(np.shape(wlen), float(bias["value"]))


def stored_16bit(values):
    """what a table stored in 16 bits holds (FunctionFromTable.cxx:183-207): multiples of (largest - smallest) / 65535 above the
    smallest entry, truncated.  It is the medium's DATA as the reference keeps it, so the statement starts from it."""
    v = np.asarray(values, dtype=np.float64)
    lo, hi = v.min(), v.max()
    return lo + np.floor(65535.0 * (v - lo) / (hi - lo)) * ((hi - lo) / 65535.0)


def absorption_lengths_of_layers(medium, wlen):
    """the absorption length of every layer at one wavelength, for the three kinds of media"""
    n = int(medium["num_layers"])
    if medium["len_mode"] == "constant":
        return np.asarray(medium["abs_const"], dtype=np.float64).copy()
    if medium["len_mode"] == "table":
        tb = medium["table"]
        grid = tb["start"] + tb["step"] * np.arange(tb["n"])
        rows = [stored_16bit(row) if tb["store16"] else np.asarray(row, dtype=np.float64) for row in tb["abs"]]
        return np.array([np.interp(float(wlen), grid, row) for row in rows])
    return icecube_absorption_length(medium, np.arange(n), float(wlen))


# ---------------------------------------------------------------------------------------------------------------------------------
# (a), (b): the first DOM on a ray
# ---------------------------------------------------------------------------------------------------------------------------------

def ray_directions(theta, phi):
    """the step direction of a flasher step (propagation_kernel.c.cl:174-182 keeps it): from the float32 angles, in float64"""
    t, p = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    return np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], axis=1)


def dom_position_error(geom):
    """delta_c of the rounding model: how far the reference's stored DOM positions may lie from the geometry's (GeometrySource.cxx:
    499-709).  Per axis: one 16 bit quantum of the largest offset from a string's mean, the template tolerance of 1e-4 m, float
    roundings of mean and z; x, y and z together in quadrature would be tighter, the plain sum is used."""
    x, y, z = (np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z"))
    sid = np.asarray(geom["string_ids"])
    sub = np.asarray([str(s) for s in geom["subdetectors"]])
    qx = qy = 0.0
    for key in set(zip(sid.tolist(), sub.tolist())):
        sel = (sid == key[0]) & (sub == key[1])
        qx = max(qx, np.abs(x[sel] - x[sel].mean()).max())
        qy = max(qy, np.abs(y[sel] - y[sel].mean()).max())
    coord = max(np.abs(x).max(), np.abs(y).max(), np.abs(z).max())
    return (qx + qy) / 32767.0 + 3e-4 + 6.0 * U * coord


def disc_error(r2, R, delta_c):
    """E of the rounding model, (1)"""
    return K_DISC * U * np.maximum(r2, 1.0) + 2.0 * R * (delta_c + 9.0 * U * np.sqrt(r2))


def first_dom(geom, p, d, pancake=1.0, chunk_elements=1 << 22):
    """For every ray (p[i], d[i]) the first DOM on it by brute force, and whether rounding decides (fragile).  Returns a dict of
    arrays: hit (bool), dom (index into the geometry's arrays, -1), s, disc, r2 (of the hit), delta_s, fragile, vertical, inside
    (the ray starts clearly inside some DOM), n_candidates (DOMs whose entry clearly lies ahead)."""
    c = np.stack([np.asarray(geom[k], dtype=np.float64) for k in ("x", "y", "z")], axis=1)
    R = float(geom["om_radius"])
    delta_c = dom_position_error(geom)
    n = len(p)
    out = dict(hit=np.zeros(n, bool), dom=np.full(n, -1), s=np.full(n, np.inf), disc=np.zeros(n), r2=np.zeros(n), delta_s=np.zeros(n),
               fragile=np.zeros(n, bool), inside=np.zeros(n, bool), n_candidates=np.zeros(n, int))
    out["vertical"] = (d[:, 0] ** 2 + d[:, 1] ** 2) == 0.0
    step = max(1, chunk_elements // len(c))
    cc = np.einsum("ij,ij->i", c, c)
    for lo in range(0, n, step):
        sl = slice(lo, min(lo + step, n))
        # |c - p|^2 and (c - p) . d through matrix products: in float64 the cancellation costs ~1e-10 m^2 at 1 km, far below E
        pc, dc = p[sl] @ c.T, d[sl] @ c.T
        r2 = np.maximum(cc[None, :] - 2.0 * pc + np.einsum("ij,ij->i", p[sl], p[sl])[:, None], 0.0)
        b = dc - np.einsum("ij,ij->i", p[sl], d[sl])[:, None]
        disc = b * b - r2 + R * R
        # every DOM is looked at; all that follows needs only those whose sphere the LINE comes near (disc > -E), a few per ray
        rows, cols = np.nonzero(disc > -disc_error(r2, R, delta_c))
        rows, r2, b, disc = rows + lo, r2[rows, cols], b[rows, cols], disc[rows, cols]
        E = disc_error(r2, R, delta_c)
        root = np.sqrt(np.maximum(disc, 0.0)) / pancake
        s, ex = b - root, b + root
        margin = delta_c + 14.0 * U * np.sqrt(r2)
        # delta_s, (2); where the line clearly crosses the sphere
        clear_line = disc >= E
        ds = np.where(clear_line, E / (2.0 * pancake * np.sqrt(np.maximum(disc, E))), np.inf) + margin
        cand = clear_line & (s >= ds) & (ex >= ds)
        # decided by rounding: a disc near zero on a DOM that is not clearly behind, an entry or exit near zero
        near_disc = (np.abs(disc) < E) & (b + np.sqrt(np.maximum(disc, 0.0) + E) / pancake + margin >= 0.0)
        near_zero = clear_line & (((np.abs(s) < ds) & (ex > -ds)) | (np.abs(ex) < ds))
        out["fragile"][rows[near_disc | near_zero]] = True
        out["inside"][rows[clear_line & (s < -ds) & (ex > ds)]] = True
        out["n_candidates"] += np.bincount(rows[cand], minlength=n)
        # the candidates of every ray in the order of their entry distances: the first is the hit, the second must be clearly behind it
        k = np.flatnonzero(cand)
        k = k[np.lexsort((s[k], rows[k]))]
        is_first = np.concatenate([[True], rows[k][1:] != rows[k][:-1]]) if len(k) else np.zeros(0, bool)
        f = k[is_first]
        out["hit"][rows[f]], out["dom"][rows[f]], out["s"][rows[f]] = True, cols[f], s[f]
        out["disc"][rows[f]], out["r2"][rows[f]], out["delta_s"][rows[f]] = disc[f], r2[f], ds[f]
        second = np.flatnonzero(~is_first)
        second = second[is_first[second - 1]]                      # the entry right after a first one, of the same ray
        close = s[k[second]] - s[k[second - 1]] < ds[k[second]] + ds[k[second - 1]]
        out["fragile"][rows[k[second[close]]]] = True
    v = out["vertical"]
    out["hit"][v], out["dom"][v], out["s"][v], out["fragile"][v] = False, -1, np.inf, False
    out["delta_c"], out["R"] = delta_c, R
    return out


def never_masked(geom):
    """Without STOP_PHOTONS_ON_DETECTION the reference marks every string and every DOM it has TESTED in a bit mask, and its `1 <<
    n` is a 32 bit shift: strings (DOMs) n and n + 32 of one 64 bit word share a bit (sparse_collision_kernel.c.cl:85-104, 245-253;
    oracle/clsim_oracle.c: opencl_int_bit), so a string or DOM is skipped when its partner was tested first -- hit or not.  Which
    partner comes first is the search's business; what can be said from the geometry alone is who HAS no partner that could come
    first.  Returns a bool per DOM: its string has no partner (the mask is per subdetector; strings count in the order of (string
    id, subdetector name)), and no partner DOM of its string lies lower (a string's layers are walked upward)."""
    sid = np.asarray(geom["string_ids"])
    sub = np.asarray([str(s) for s in geom["subdetectors"]])
    z = np.asarray(geom["z"], dtype=np.float64)
    keys = sorted(set(zip(sid.tolist(), sub.tolist())))
    rank = {k: i for i, k in enumerate(keys)}
    free = np.zeros(len(sid), bool)
    for key in keys:
        s = rank[key]
        partner = any(k[1] == key[1] and rank[k] != s and rank[k] // 64 == s // 64 and rank[k] % 32 == s % 32 for k in keys)
        members = np.flatnonzero((sid == key[0]) & (sub == key[1]))
        for n, i in enumerate(members):
            lower = any(m != n and m // 64 == n // 64 and m % 32 == n % 32 and z[j] < z[i] for m, j in enumerate(members))
            free[i] = not partner and not lower
    return free


def intersection(c, R, delta_c, q, d, pancake):
    """one known DOM per ray: (b, disc, s, E, delta_s) of statement (a) for centre c[i], start q[i], direction d[i]"""
    rel = c - q
    r2 = np.einsum("ij,ij->i", rel, rel)
    b = np.einsum("ij,ij->i", rel, d)
    disc = b * b - r2 + R * R
    E = disc_error(r2, R, delta_c)
    s = b - np.sqrt(np.maximum(disc, 0.0)) / pancake
    ds = E / (2.0 * pancake * np.sqrt(np.maximum(disc, E))) + delta_c + 14.0 * U * np.sqrt(r2)
    return b, disc, s, E, ds


def expected_hit_position(c, q, d, s, pancake):
    """saveHit (propagation_kernel.c.cl:307-404): the hit point relative to the DOM, whose centre is shifted by (1 - 1/pancake) of
    the start point's offset perpendicular to the ray.  It lies on the sphere of radius R / pancake."""
    off = q - c
    perp = off - np.einsum("ij,ij->i", off, d)[:, None] * d
    centre = c + (1.0 - 1.0 / pancake) * perp
    return q + s[:, None] * d - centre


def weight_bound(bias, wlen):
    """relative: weight = w / bias(wavelength) with the bias table interpolated in float32 (FunctionFromTable.cxx:213-291): the bin
    coordinate q = (wavelength - start) / step carries the literals' and its own roundings, 4 u q absolute in the fraction, which the
    table's slope passes on; the two entries, their difference, the mix and the division 5 u"""
    v = np.asarray(bias["values"], dtype=np.float64)
    q = (np.asarray(wlen, dtype=np.float64) - bias["start"]) / bias["step"]
    k = np.clip(np.floor(q).astype(int), 0, len(v) - 2)
    return U * (5.0 + 4.0 * np.abs(q) * np.abs(v[k + 1] - v[k]) / table_value(bias, wlen))


def angle_bounds(theta):
    sin_t = np.maximum(np.abs(np.sin(np.asarray(theta, dtype=np.float64))), 1e-30)
    return U * (8.0 + 8.0 / sin_t) + 2.0 * ulp32(math.pi), 8.0 * U / sin_t + 2.0 * ulp32(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c): absorption lengths used up on a straight segment
# ---------------------------------------------------------------------------------------------------------------------------------

DZ_SMALL = 2e-5
A0_MAX = -math.log(U)            # abs_lens_initial = -ln(uniform in (0, 1]), the smallest uniform is 2^-24: at most 16.64


def absorption_lengths_used(medium, p0, p1, wlen, lengths=None):
    """The absorption lengths a photon of wavelength wlen uses up between p0 and p1, as the reference defines them
    (propagation_kernel.c.cl:600-700; oracle/clsim_oracle.c:1014-1065):
      * shift = tilt(p0), taken ONCE at the start; the whole segment walks in z - shift;
      * layer l spans layer_bottom + l thickness upward, the outermost layers extend to infinity;
      * sum over the layers crossed of (path in the layer) / absLen(l, wlen), where path in layer = L (delta z in layer) / |delta z|;
      * divided by the anisotropy factor of the segment's direction.
    For |dz| < 1e-5 the reference uses ONE layer's lengths for the whole segment (oracle/clsim_oracle.c:1050: `if ((currentPhotonLayer
    == j) || (fabs(photon_dz) < EPSILON))`); such segments (|dz| < DZ_SMALL, flag `flat`) are left out of comparisons.

    Returns (used, bound, flat, crossings).  The bound, first order in u:
      * arithmetic of the budget: every quantity of the walk (abs_lens_left, ais/aia times thickness) is at most abs_lens_initial
        =: A0 in absorption lengths; one trip rounds it about ten times (scaling by the anisotropy factor and back, the two
        products and the quotient of aia, distanceToAbsorption, the remainder's subtraction and quotient, the history's
        subtraction at both ends) and once per layer crossed (aia += 1 / absLen): u A0 (crossings + 10).  A0 is not in a record;
        A0 <= A0_MAX = 16.64.
      * the end points are float32 (half an ulp of ~600 m per coordinate) and the reference's direction is a unit vector to ~4 u:
        the length moves by sqrt(3) ulp(M), the direction by sqrt(3) ulp(M) / L, which the anisotropy factor (|d ln f / d angle| <
        0.5) passes on: 1.5 sqrt(3) ulp(M) / (min absLen on the segment).
      * a layer boundary, in z - shift, is known to delta_z = 4 ulp(M) (z, the float32 tilt -- bilinear in values below 100 m --,
        the boundary's own product and sum): path delta_z L / |delta z| moves from one layer to its neighbour, at every boundary
        crossed and at both ends (a point within delta_z of a boundary may be taken for the other layer):
        delta_z (L / |delta z|) sum |1 / absLen_a - 1 / absLen_b|.
    All of it divided by the anisotropy factor."""
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    seg = p1 - p0
    L = float(np.linalg.norm(seg))
    M = float(max(np.abs(p0).max(), np.abs(p1).max(), 1.0))
    n = int(medium["num_layers"])
    bottom, th = float(medium["layers_z_start"]), float(medium["layers_height"])
    if lengths is None:                 # (the caller may hold absorption_lengths_of_layers(medium, wlen) for many segments)
        lengths = absorption_lengths_of_layers(medium, wlen)
    factor = 1.0
    if "aniso" in medium and L > 0.0:
        an = medium["aniso"]
        factor = float(ppc_anisotropy((seg / L)[None, :], an["azimuth"], an["k1"], an["k2"])[0])
    shift = float(tilt_independent(medium, p0[None, :])[0]) if "tilt" in medium else 0.0
    za, zb = p0[2] - shift, p1[2] - shift
    dz = zb - za
    flat = L == 0.0 or abs(dz) / max(L, 1e-300) < DZ_SMALL
    lo, hi = min(za, zb), max(za, zb)
    layer_of = lambda z: int(min(max(math.floor((z - bottom) / th), 0), n - 1))
    la, lb = layer_of(lo), layer_of(hi)
    delta_z = 4.0 * float(ulp32(M))
    if la == lb or flat:
        used = L / lengths[layer_of(za)]
        crossings = 0
        edge = 0.0
    else:
        edges = bottom + th * np.arange(la + 1, lb + 1)            # the boundaries between layers la .. lb
        cuts = np.concatenate([[lo], edges, [hi]])
        used = float(np.sum(np.diff(cuts) / lengths[la:lb + 1])) * (L / abs(dz))
        crossings = lb - la
        edge = float(np.sum(np.abs(np.diff(1.0 / lengths[la:lb + 1]))))
    # both ends may sit within delta_z of a boundary
    for z in (lo, hi):
        k = layer_of(z)
        for other, boundary in ((k - 1, bottom + th * k), (k + 1, bottom + th * (k + 1))):
            if 0 <= other < n and abs(z - boundary) <= delta_z:
                edge += abs(1.0 / lengths[k] - 1.0 / lengths[other])
    slope = L / abs(dz) if abs(dz) > 0 else 0.0
    bound = U * A0_MAX * (crossings + 10) + 1.5 * math.sqrt(3.0) * float(ulp32(M)) / float(lengths[la:lb + 1].min()) + delta_z * slope * edge
    return used / factor, bound / factor, flat, crossings
