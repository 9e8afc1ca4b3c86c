"""Inputs shared by the CPU and the GPU tests of the sub-pixel refinement: analytic images with known shifts, and one item per
status of ssba_track_refine at its boundary.  The expected statuses are stated here by hand; test_tracks_refine_reference.py
holds the numpy statement to them and test_gpu_tracks_subpixel.py the device to the statement."""
import functools

import numpy as np

import tracks_refine_reference as rr

SHIFTS = [(0.3, 0.0), (0.5, 0.25), (1.4, -0.7), (2.6, 1.5), (-3.3, 0.8), (3.75, -3.2), (0.0, 0.0)]


@functools.lru_cache(maxsize=None)
def sinusoids(rows, cols, shift=(0.0, 0.0), seed=3, noise=0, y_only=False):
    """A sum of six sinusoids with wavelengths of 8 to 24 pixels, displaced by `shift` = (sx, sy): what image (x, y) of the
    unshifted call shows, this one shows at (x + sx, y + sy).  noise: uniform integer grey levels in [-noise, noise]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    img = np.full((rows, cols), 128.0)
    for _ in range(6):
        wavelength, angle, phase = rng.uniform(8.0, 24.0), rng.uniform(0.0, np.pi), rng.uniform(0.0, 2 * np.pi)
        if y_only:
            angle = np.pi / 2
        img += 18.0 * np.sin(2 * np.pi / wavelength * (np.cos(angle) * x + np.sin(angle) * y) + phase)
    if noise:
        img += np.random.Generator(np.random.PCG64(seed + 1000 + int(1000 * abs(shift[0]) + 7 * abs(shift[1])))).integers(-noise, noise + 1, img.shape)
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


STATUS_IMAGES = ("texture", "half", "constant", "rows", "minus_one", "minus_one_and_half", "two", "noisy")


@functools.lru_cache(maxsize=None)
def status_stack(rows=40, cols=56):
    t = sinusoids(rows, cols)
    stack = np.stack([t, sinusoids(rows, cols, (0.5, 0.0)), np.full((rows, cols), 90, np.uint8), sinusoids(rows, cols, y_only=True),
                      sinusoids(rows, cols, (-1.0, -1.0)), sinusoids(rows, cols, (-1.5, 0.0)), sinusoids(rows, cols, (2.0, 0.0)),
                      sinusoids(rows, cols, (0.5, 0.0), noise=2)])
    stack.setflags(write=False)
    return stack


def status_cases(rows=40, cols=56):
    """(name, item, refine parameters, expected status) with the images of status_stack(rows, cols).  The integer shifts are exact
    copies (the same function sampled at the same points), so there the truth is a zero of the residual and is reached exactly."""
    I = {n: k for k, n in enumerate(STATUS_IMAGES)}
    cx, cy = cols // 2, rows // 2
    q = 256
    cases = [
        ("anchor support leaves the image", [I["texture"], 7, cy, I["texture"], q * cx, q * cy, 0], {}, rr.EDGE),
        ("anchor support just inside", [I["texture"], 8, 8, I["texture"], q * 8, q * 8, 0], {}, rr.OK),
        ("anchor support leaves at the far corner", [I["texture"], cols - 8, rows - 9, I["texture"], q * cx, q * cy, 0], {}, rr.EDGE),
        ("anchor support just inside the far corner", [I["texture"], cols - 9, rows - 9, I["texture"], q * (cols - 9), q * (rows - 9), 0], {}, rr.OK),
        ("start window just inside", [I["texture"], 8, 8, I["minus_one"], q * 7, q * 7, 0], {}, rr.OK),
        ("start window leaves the image", [I["texture"], 8, 8, I["minus_one"], q * 7 - 1, q * 7, 0], {}, rr.EDGE),
        ("start window leaves in y, x only", [I["texture"], 8, 8, I["minus_one"], q * 7, q * 7 - 1, 1], {}, rr.EDGE),
        ("window leaves after a step", [I["texture"], 8, cy, I["minus_one_and_half"], q * 7, q * cy, 0], {}, rr.EDGE),
        ("window leaves after a step, x only", [I["texture"], 8, cy, I["minus_one_and_half"], q * 7, q * cy, 1], {}, rr.EDGE),
        ("constant patch", [I["constant"], cx, cy, I["texture"], q * cx, q * cy, 0], {}, rr.FLAT),
        ("constant patch, x only", [I["constant"], cx, cy, I["texture"], q * cx, q * cy, 1], {}, rr.FLAT),
        ("texture of rows, x only", [I["rows"], cx, cy, I["rows"], q * cx, q * cy, 1], {}, rr.FLAT),
        ("texture of rows, 2-D: singular", [I["rows"], cx, cy, I["rows"], q * cx, q * cy, 0], {}, rr.FLAT),
        ("moved by max_shift exactly", [I["texture"], cx, cy, I["two"], q * cx, q * cy, 0], dict(max_shift=2), rr.OK),
        ("moved one unit beyond max_shift", [I["texture"], cx, cy, I["two"], q * cx - 1, q * cy, 0], dict(max_shift=2), rr.FAR),
        ("moved by max_shift exactly, x only", [I["texture"], cx, cy, I["two"], q * cx, q * cy, 1], dict(max_shift=2), rr.OK),
        ("moved one unit beyond max_shift, x only", [I["texture"], cx, cy, I["two"], q * cx - 1, q * cy, 1], dict(max_shift=2), rr.FAR),
        ("one evaluation at half a pixel", [I["texture"], cx, cy, I["half"], q * cx, q * cy, 0], dict(iterations=1), rr.ITERATIONS),
        ("enough evaluations at half a pixel", [I["texture"], cx, cy, I["half"], q * cx, q * cy, 0], {}, rr.OK),
    ]
    # the SAD gate at the sad itself and one below: the sad of the ungated run, which the numpy statement supplies
    item = [I["texture"], cx, cy, I["noisy"], q * cx, q * cy, 0]
    _, _, status, sad = rr.refine_one(status_stack(rows, cols)[item[0]], item[1], item[2], status_stack(rows, cols)[item[3]], item[4], item[5], item[6])
    assert status == rr.OK and sad >= 2, (status, sad)
    cases += [("sad equal to max_sad", item, dict(max_sad=sad), rr.OK), ("sad one above max_sad", item, dict(max_sad=sad - 1), rr.SAD)]
    return cases
