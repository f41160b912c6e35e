"""numpy restatement of the ray queries' slab parts (include/rgbd_recon_hip.h, "ray queries: slab parts"), on top of tests/ray_reference.py's setup.

trace() follows every ray through ALL its max_n samples once -- positions by the chained additions, densities through the oracle's sampling primitive, the
owner plane of every sample by the header's formula.  The whole-volume answer (the first sample with dens > 0) and every slab's part (the first such
sample among those the slab owns) are then read off the trace by one function, so a case costs one pass however many slabs it has.  merge() is the
header's merge rule, and seam_rays() generates rays that exercise every seam of a slab set."""
import numpy as np

import ray_reference as Q

f32 = np.float32


def owner_plane(z, rz):
    """fminf(fmaxf(floorf(z * (float)rz), 0.0f), (float)(rz - 1)) as an integer: fmaxf / fminf drop a NaN (plane 0), +-inf clamp"""
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(z, f32) * f32(rz)).astype(f32))
        return np.fmin(np.fmax(f, f32(0.0)), f32(rz - 1)).astype(np.int64)


def trace(vol, limit, bbox_min, bbox_max, rays, unit_cube):
    """-> dict(S=ray_reference.setup's result, pos [n][K][3], dens [n][K], plane [n][K] int, live [n][K] bool (k < max_n)), K = the longest ray's max_n"""
    rays = np.asarray(rays)
    S = Q.setup(rays, limit, bbox_min, bbox_max, unit_cube)
    n, K = len(rays), int(S["max_n"].max()) if len(rays) else 0
    rz = np.asarray(vol).shape[0]
    tex = Q.Sampler(vol)
    pos = np.zeros((n, K, 3), f32)
    dens = np.zeros((n, K), f32)
    p, step = S["pos"].copy(), S["step"]
    with np.errstate(all="ignore"):
        for k in range(K):
            pos[:, k] = p
            for i in np.nonzero(S["max_n"] > k)[0]:
                dens[i, k] = tex(p[i])
            p = (p + step).astype(f32)
        plane = owner_plane(pos[:, :, 2], rz)
    live = np.arange(K)[None, :] < S["max_n"][:, None]
    return dict(S=S, pos=pos, dens=dens, plane=plane, live=live, limit=f32(limit), unit_cube=bool(unit_cube),
                lo=np.asarray(bbox_min, f32), ext=(np.asarray(bbox_max, f32) - np.asarray(bbox_min, f32)).astype(f32))


def owner(T, slabs):
    """[n][K]: the index of the slab (voxel planes [z0, z1), tile aligned) that owns each sample, by plane >> 3 in [z0 / 8, (z1 + 7) / 8)"""
    layer = T["plane"] >> 3
    out = np.full(layer.shape, -1, np.int64)
    for s, (z0, z1) in enumerate(slabs):
        out[(layer >= z0 // 8) & (layer < (z1 + 7) // 8)] = s
    assert (out >= 0).all()                                              # contiguous slabs that cover the volume own every sample
    return out


def first_hit(T, examined):
    """[n]: the smallest k with dens_k > 0 among the live samples marked in `examined` [n][K], -1 where there is none"""
    with np.errstate(invalid="ignore"):
        m = examined & T["live"] & (T["dens"] > 0)                       # (a NaN density compares as no hit)
    return np.where(m.any(1), m.argmax(1), -1) if m.shape[1] else np.full(len(m), -1, np.int64)


def answer(T, k):
    """the record of a march that stopped at sample k [n] (-1: no hit) -> dict(hits RAY_HIT_DTYPE [n], unit [n][3]); prev is sample k - 1's density"""
    S = T["S"]
    n = len(k)
    hits = np.zeros(n, Q.RAY_HIT_DTYPE)
    unit = np.zeros((n, 3), f32)
    hit = k >= 0
    i = np.nonzero(hit)[0]
    ki = k[i]
    with np.errstate(all="ignore"):
        d = T["dens"][i, ki]
        prev = np.where(ki > 0, T["dens"][i, np.maximum(ki - 1, 0)], -T["limit"]).astype(f32)
        kk = (prev / (d - prev)).astype(f32)
        p, step = T["pos"][i, ki], S["step"][i]
        unit[i] = ((p - step) - step * kk[:, None]).astype(f32)
        o, dd = S["o"], S["d"]
        t = ((unit[:, 0] - o[:, 0]) * dd[:, 0] + (unit[:, 1] - o[:, 1]) * dd[:, 1] + (unit[:, 2] - o[:, 2]) * dd[:, 2]).astype(f32) / S["len2"]
        world = unit if T["unit_cube"] else (T["lo"][None, :] + unit * T["ext"][None, :]).astype(f32)
    hits["pos"] = np.where(hit[:, None], world, f32(0.0))
    hits["t"] = np.where(hit, t, f32(-1.0))
    hits["n_samples"] = np.where(hit, k + 1, S["max_n"])
    hits["status"] = S["status"] | np.where(hit, Q.HIT, 0).astype(np.uint32)
    return dict(hits=hits, unit=unit)


def whole(T):
    """the whole-volume cast: ray_reference.cast's result, read off the trace"""
    return answer(T, first_hit(T, np.ones(T["live"].shape, bool)))


def parts(T, slabs):
    """one answer() per slab: the first hit among the samples the slab owns"""
    own = owner(T, slabs)
    return [answer(T, first_hit(T, own == s)) for s in range(len(slabs))]


def stored_planes(rz, limit, slab):
    """voxel planes [zlo, zhi] a context of slab (z0, z1) stores: its owned tile layers and the halo, ceil((limit * rz + 2) / 8) layers to either side"""
    ntz = (rz + 7) // 8
    halo = int(np.ceil((f32(limit) * f32(rz) + f32(2.0)) / f32(8.0)))
    tz0, tz1 = slab[0] // 8, (slab[1] + 7) // 8
    whole = tz0 == 0 and tz1 == ntz
    lo, hi = (0, ntz) if whole else (max(0, tz0 - halo), min(ntz, tz1 + halo))
    return lo * 8, min(hi * 8, rz) - 1


def part_volume(vol, limit, slab):
    """the volume as a slab context's taps read it: every z tap is clamped into the stored planes, i.e. the planes outside repeat the nearest stored one"""
    vol = np.asarray(vol, f32)
    zlo, zhi = stored_planes(vol.shape[0], limit, slab)
    out = vol.copy()
    out[:zlo] = vol[zlo]
    out[zhi + 1:] = vol[zhi]
    return out


def part_surface(vol, scene, limit, bbox_min, bbox_max, part, slab, normals=True, colours=True):
    """the surface records of a part: ray_reference.surface on the slab's stored planes.  For a record that can win the merge (prev <= 0 < dens) the
    refined point lies within one step behind the owned sample and the halo covers its taps, so this is the whole volume's surface; a part hit whose
    predecessor was itself a hit (in the neighbour's slab: it never wins) refines to anywhere on the ray, where the clamp shows."""
    return Q.surface(part_volume(vol, limit, slab), scene, limit, bbox_min, bbox_max, part, normals=normals, colours=colours)


def merge(part_hits, part_surfaces=None):
    """the merge rule: per ray the part with HIT and the smallest n_samples, part 0 when none hit; the surface travels with the winner"""
    n = len(part_hits[0])
    win = np.zeros(n, np.int64)
    best = np.full(n, np.iinfo(np.int64).max)
    for s, h in enumerate(part_hits):
        ns = h["n_samples"].astype(np.int64)
        better = ((h["status"] & Q.HIT) != 0) & (ns < best)
        assert not (((h["status"] & Q.HIT) != 0) & (ns == best)).any()   # no two parts tie: a sample has one owner
        win[better], best[better] = s, ns[better]
    hits = np.stack(part_hits)[win, np.arange(n)]
    if part_surfaces is None:
        return hits, win
    return hits, np.stack(part_surfaces)[win, np.arange(n)], win


# ---------------------------------------------------------------------------------------------------------------- rays
def seam_rays(seed, res, slabs, vol, limit, n_total=2000, per_seam=130):
    """Rays in the unit cube's frame for a slab set: test_gpu_rays.ray_mix (outside, inside, inside the surface, misses, axis-parallel, un-normalised,
    finite intervals, every invalid kind); rays with dz = 0 at z exactly on each seam plane and half a voxel to either side; +-z axis rays through all
    slabs; origins inside each slab pointing up and down, many of them a few steps from a seam so that a march crosses it before it ends; intervals
    that begin in one slab and end in another."""
    from test_gpu_rays import ray_mix
    rx, ry, rz = res
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.nonzero(np.nan_to_num(np.asarray(vol), nan=-1.0) > 0)
    inside = np.stack([(xx + 0.5) / rx, (yy + 0.5) / ry, (zz + 0.5) / rz], 1)
    out = []
    sd = limit * 0.5
    seams = [z1 / rz for _, z1 in slabs[:-1]]

    def jitter(n, spread):
        d = rng.normal(size=(n, 3)) * spread
        return d

    for zs in seams:
        for dz in (0.0, -0.5 / rz, 0.5 / rz):                            # in the seam plane, and half a voxel to either side: dz = 0
            n = 16
            o = np.column_stack([np.where(rng.random(n) < 0.5, -0.2, rng.uniform(0.1, 0.9, n)), rng.uniform(0.1, 0.9, n), np.full(n, zs + dz)])
            d = np.column_stack([rng.uniform(0.2, 1.0, n), rng.uniform(-0.5, 0.5, n), np.zeros(n)])
            out.append(Q.make_rays(o, d))
        for sign in (1.0, -1.0):                                         # a few steps in front of the seam, pointing across it
            n = per_seam
            back = rng.uniform(0.0, 2.5, n) * sd
            o = np.column_stack([rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), zs - sign * back])
            d = jitter(n, 0.25)
            d[:, 2] = sign * rng.uniform(0.6, 1.4, n)
            out.append(Q.make_rays(o, d * rng.uniform(0.2, 3.0, (n, 1))))
            m = 24                                                       # an interval that begins in one slab and ends in the other
            o = np.column_stack([rng.uniform(0.2, 0.8, m), rng.uniform(0.2, 0.8, m), np.full(m, zs - sign * 0.6)])
            d = np.zeros((m, 3))
            d[:, 2] = sign * rng.uniform(0.5, 2.0, m)
            t0 = (0.6 - rng.uniform(0.2, 2.0, m) * sd) / np.abs(d[:, 2])
            t1 = (0.6 + rng.uniform(0.5, 6.0, m) * sd) / np.abs(d[:, 2])
            out.append(Q.make_rays(o, d, t0, t1))
    n = 40                                                               # +-z axis rays through all slabs
    xy = rng.uniform(0.05, 0.95, (n, 2))
    up = rng.random(n) < 0.5
    out.append(Q.make_rays(np.column_stack([xy, np.where(up, -0.3, 1.3)]), np.column_stack([np.zeros((n, 2)), np.where(up, 1.0, -1.0)])))
    for z0, z1 in slabs:                                                 # origins inside each slab, pointing up and down
        n = 40
        o = np.column_stack([rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(z0 / rz, z1 / rz, n)])
        d = jitter(n, 0.3)
        d[:, 2] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        out.append(Q.make_rays(o, d))
    n_mix = max(512, n_total - sum(len(r) for r in out))                  # the mix fills the case up to about n_total rays
    return np.concatenate([ray_mix(seed, n_mix, inside, (0, 0, 0), (1, 1, 1), False)] + out)


def seam_counts(T, slabs):
    """per seam s (between slabs s and s + 1): dict(elsewhere: rays whose winning hit lies in another slab than their first sample, on either side of the
    seam; predecessor: rays whose hit's predecessor sample belongs to the slab across the seam; downward: rays with dz < 0 whose march crosses the seam
    before it ends), and two_hits: rays that hit in more than one slab (so the minimum decides)"""
    own = owner(T, slabs)
    k = first_hit(T, np.ones(T["live"].shape, bool))
    i = np.nonzero(k >= 0)[0]
    o_first, o_hit = own[i, 0], own[i, k[i]]
    o_prev = own[i, np.maximum(k[i] - 1, 0)]
    last = np.where(k >= 0, k, T["S"]["max_n"].astype(np.int64) - 1)     # the last sample the whole march takes
    marched = T["live"] & (np.arange(own.shape[1])[None, :] <= last[:, None])
    down = T["S"]["step"][:, 2] < 0
    per = []
    for s in range(len(slabs) - 1):
        lo, hi = np.minimum(o_first, o_hit), np.maximum(o_first, o_hit)
        crossed = (marched & (own == s)).any(1) & (marched & (own == s + 1)).any(1)
        per.append(dict(elsewhere=int(((lo <= s) & (hi > s)).sum()),
                        predecessor=int(((k[i] > 0) & (np.minimum(o_prev, o_hit) == s) & (np.maximum(o_prev, o_hit) == s + 1)).sum()),
                        downward=int((down & crossed).sum())))
    part_hits = np.stack([first_hit(T, own == s) >= 0 for s in range(len(slabs))])
    return per, int((part_hits.sum(0) > 1).sum())
