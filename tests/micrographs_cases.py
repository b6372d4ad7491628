"""Built scenes for vk.micrographs: what tests/test_micrographs_cpu.py proves valid and tests/test_vk_micrographs_gpu.py renders.  Every
scene is a micrographs_ref.SCENE_DT record; coordinates are in 1/16 pixel."""
import numpy as np

import micrographs_ref as R


def indent(vx, vy, ax, ay, shade=(60, 95, 130, 165), slope=(-20, 12, -6, 18), ridge=35, ridge_hw=10, halo_r=48, halo_depth=24):
    q = np.zeros((), R.INDENT_DT)
    q["vx"], q["vy"], q["ax"], q["ay"], q["shade"], q["slope"] = vx, vy, ax, ay, shade, slope
    q["ridge"], q["ridge_hw"], q["halo_r"], q["halo_depth"] = ridge, ridge_hw, halo_r, halo_depth
    return q


def diamond(cx, cy, h, **kw):
    """A square on its corner, centre (cx, cy) and half diagonal h in 1/16 pixel, the apex a little off the centre."""
    return indent((cx + h, cx, cx - h, cx), (cy, cy + h, cy, cy - h), cx + h // 8, cy - h // 10, **kw)


def scratch(x, y, dx, dy, hw, depth, t0=R.I32_MIN, t1=R.I32_MAX):
    return np.array((x, y, dx, dy, hw, depth, t0, t1), R.SCRATCH_DT)


def rect(x0, y0, x1, y1, thickness, color):
    return np.array((x0, y0, x1, y1, thickness, color), R.RECT_DT)


def scene(S, indents=(), scratches=(), blobs=(), rects=(), base=150, tint=(246, 262, 238), grad=(9, -7), vig=12, tex_amp=24, theta=0.6, blur_r=0,
          noise_amp=0, seed=1):
    s = R.blank_scene(base, tint)
    s["grad_x"], s["grad_y"], s["grad_cx"], s["grad_cy"] = grad[0], grad[1], S // 2, S // 2 + 1
    s["vig"], s["vig_cx"], s["vig_cy"] = vig, S // 2 - 3, S // 2 + 2
    s["tex_amp"], s["tex_cos"], s["tex_sin"] = tex_amp, int(round(16384 * np.cos(theta))), int(round(16384 * np.sin(theta)))
    s["tex_lu"], s["tex_lv"], s["tex_seed"] = 3, 1, 0x9E3779B9 ^ seed
    s["blur_r"], s["noise_amp"], s["noise_seed"] = blur_r, noise_amp, 0xC0FFEE00 + seed
    for name, lst in (("indents", indents), ("scratches", scratches), ("blobs", blobs), ("rects", rects)):
        for i, r in enumerate(lst):
            s[name][i] = r
        s["n_" + name] = len(lst)
    return s


def full_scene(S, seed, blur_r=3):
    """Every limit reached at once: 8 indentations on a 4 x 2 grid, 64 scratches, 8 blobs, 4 rects."""
    rng = np.random.default_rng([seed, S])
    px, py = S * 16 // 4, S * 16 // 2
    h = min(px, py) // 2 - 8
    ind = [diamond(px // 2 + (k % 4) * px + int(rng.integers(-4, 5)), py // 2 + (k // 4) * py + int(rng.integers(-4, 5)), h, halo_r=16 + k,
                   ridge_hw=4 + k, ridge=(-40, 40)[k & 1]) for k in range(8)]
    scr = []
    for k in range(64):
        a = rng.uniform(0, np.pi)
        fin = k % 3 == 0
        ext = int(rng.integers(1, 16 * S)) * 16384
        scr.append(scratch(int(rng.integers(0, 16 * S)), int(rng.integers(0, 16 * S)), int(round(16384 * np.cos(a))), int(round(16384 * np.sin(a))),
                           int(rng.integers(0, 24)), int(rng.integers(-30, 31)), -ext if fin else R.I32_MIN, ext // 2 if fin else R.I32_MAX))
    blobs = [np.array((int(rng.integers(0, 16 * S)), int(rng.integers(0, 16 * S)), int(rng.integers(16, 16 * 5)), int(rng.integers(10, 90))), R.BLOB_DT)
             for _ in range(8)]
    rects = [rect(1, 2, S - 3, S - 4, 1, (0, 0, 255)), rect(S // 2, S // 2, S + 5, S + 5, 0, (16, 16, 16)), rect(S // 2 + 1, S - 3, S - 2, S - 2, 0, (255, 255, 255)),
             rect(-5, -5, 2, 1, 2, (0, 255, 0))]
    return scene(S, ind, scr, blobs, rects, blur_r=blur_r, noise_amp=9, seed=seed)


def last_row_col_rects(S):
    return [rect(0, S - 1, S - 1, S - 1, 0, (255, 0, 0)), rect(S - 1, 0, S - 1, S - 2, 0, (0, 255, 0)), rect(2, 2, S - 1, S - 1, 1, (0, 0, 255))]


def render_cases():
    """(name, S, [scenes]): the sizes and records of the issue."""
    cases = []
    cases.append(("S16 no records", 16, [R.blank_scene(131, (256, 200, 300))]))
    # a vertex on a pixel centre (16 * 12, 16 * 6) and an edge through pixel centres, smaller than a tile, every optic on
    cases.append(("S16 one indentation", 16, [scene(16, [diamond(16 * 6, 16 * 6, 16 * 6, halo_r=40)], [scratch(40, 40, 16384, 0, 3, -30)], blur_r=3, noise_amp=7,
                                                    rects=last_row_col_rects(16))]))
    cases.append(("S20 scalar stores", 20, [scene(20, blur_r=1, noise_amp=4), scene(20, [diamond(170, 150, 90)], [scratch(10, 200, 11585, 11585, 5, 25)],
                                                                                     rects=last_row_col_rects(20), blur_r=2, seed=2),
                                            full_scene(20, 3)]))
    s80 = [
        # straddling the tile corner (64, 16) in pixels; blur 0
        scene(80, [diamond(16 * 64 + 5, 16 * 16 - 3, 16 * 11 + 7), diamond(16 * 30, 16 * 60, 16 * 9)],
              [scratch(16 * 40, 16 * 40, 15137, 6270, 3, -28), scratch(16 * 10, 16 * 70, 16069, -3196, 16 * 5, 14), scratch(16 * 50, 16 * 8, 0, 16384, 9, -20, -16 * 16384 * 20, 0)],
              [np.array((16 * 70 + 3, 16 * 40 + 9, 60, 70), R.BLOB_DT)], blur_r=0, noise_amp=5, seed=4),
        # clipped by the image border on two sides, a vertex on the pixel centre (20, 0); blur 3
        scene(80, [indent((16 * 20, 16 * 30 + 7, 16 * 2 + 1, -16 * 6 - 5), (16 * 0, 16 * 12 + 3, 16 * 31, 16 * 14), 16 * 10, 16 * 13, halo_r=16 * 4),
                   indent((16 * 86, 16 * 70, 16 * 55 + 8, 16 * 71), (16 * 72, 16 * 88, 16 * 71, 16 * 58), 16 * 70 + 4, 16 * 72, halo_r=0)],
              [scratch(16 * 79, 16 * 79, 11585, -11585, 7, 30)], rects=last_row_col_rects(80), blur_r=3, noise_amp=0, seed=5),
        full_scene(80, 6),
    ]
    cases.append(("S80 three scenes", 80, s80))
    cases.append(("S80 one scene", 80, [s80[1]]))
    return cases


def two_indent_scene(S=128):
    """Two well separated indentations on a plain background, for detect_gt against truth()."""
    return scene(S, [diamond(16 * 36 + 4, 16 * 40 + 8, 16 * 20 + 5, halo_r=0), indent((16 * 110, 16 * 88 + 2, 16 * 70 + 9, 16 * 90), (16 * 84, 16 * 104 + 3, 16 * 86, 16 * 66),
                                                                                   16 * 91, 16 * 85, halo_r=32)], tex_amp=0, vig=0, grad=(0, 0))
