"""The draws of the stress families 19 to 25 (tests/stress_parity.py), without a GPU and without the library: 400 cases
of each from the seed the suite's slice uses (6000 + family), so the first of them are the cases the GPU run sees.  Every
case must lie inside the operator's domain - the limits are recomputed here from the constants of the kernels' sources,
read the way tests/test_enhance_edge_sizes.py reads them - since the driver counts a declined case as a mismatch; every
value of every categorical axis must occur; and the structural targets (the rank routes of StatisticImage, an
AdaptiveThresholdImage frame over one strip and one over one band, the three kinds of geometry) must come within the first
40 cases, about what four seconds run."""
import re

import numpy as np
import pytest

import stress_parity
import clahe_oracle
import kuwahara_oracle
import levels_oracle
import scale_oracle
import statistic_oracle
import threshold_oracle
from test_enhance_edge_sizes import source, function_body

CASES, FIRST = 400, 40
_DRAWN = {}


def draws(op):
    """The first CASES cases of family `op`, drawn once and shared (read-only)."""
    if op not in _DRAWN:
        saved = stress_parity.rng, dict(stress_parity.drawn)
        stress_parity.rng = np.random.default_rng(6000 + op)
        stress_parity.drawn.clear()
        try:
            _DRAWN[op] = [stress_parity.DRAWS[op](op) for _ in range(CASES)]
        finally:
            stress_parity.rng = saved[0]
            stress_parity.drawn.clear()
            stress_parity.drawn.update(saved[1])
        for case in _DRAWN[op]:
            case["frame"].setflags(write=False)
    return _DRAWN[op]


def constant(text, name):
    m = re.search(r"constexpr\s+\w+(?:\s+\w+)?\s+%s=([^;]+);" % re.escape(name), text)
    assert m, "no constant %s" % name
    return m.group(1).strip()


def adaptive_constants():
    text = source("threshold.hip")
    threads, lanes = int(constant(text, "kAdaptiveThreads")), int(constant(text, "kAdaptiveLaneColumns"))
    assert constant(text, "kAdaptiveSpan") == "kAdaptiveThreads*kAdaptiveLaneColumns"
    assert constant(text, "kAdaptiveMaxWidth") == "kAdaptiveSpan/2+1"
    assert constant(text, "kAdaptiveFloatMaxSide") == "1 << 20"
    plan = function_body(text, "static MhStatus adaptive_plan(")
    assert "a->outputs=kAdaptiveSpan-((int) width-1);" in plan and "a->band=std::max(kAdaptiveBandRows,4*(int) height);" in plan
    span = threads * lanes
    return span, int(constant(text, "kAdaptiveBandRows")), span // 2 + 1, 1 << 20


@pytest.mark.parametrize("op", sorted(stress_parity.DRAWS))
def test_every_axis_takes_every_value(op):
    cases = draws(op)
    assert len(cases) == CASES and [case["index"] for case in cases] == list(range(CASES))
    layouts = {19: ["gray", "gray+alpha", "rgb", "rgba"], 20: ["gray", "gray+alpha", "rgb", "rgba"], 21: kuwahara_oracle.LAYOUTS,
               22: ["rgb", "rgba"], 23: threshold_oracle.LAYOUTS, 24: levels_oracle.LAYOUTS, 25: scale_oracle.LAYOUTS}[op]
    names = {19: ["statistic"], 20: ["bilateral_blur", "selective_blur"], 21: ["kuwahara"], 22: ["clahe"],
             23: stress_parity.THRESHOLD_OPERATORS, 24: stress_parity.LEVEL_OPERATORS, 25: stress_parity.SCALE_OPERATORS}[op]
    assert {case["layout"] for case in cases} == set(layouts)
    assert {case["name"] for case in cases} == set(names)
    for axis in ("float", "fast", "host"):
        assert {case[axis] for case in cases} == {False, True}, axis
    assert {case["mask"] is None for case in cases} == {False, True}
    share = {axis: np.mean([case[axis] for case in cases]) for axis in ("float", "fast", "host")}
    assert 0.4 < share["float"] < 0.6 and 0.4 < share["fast"] < 0.6 and 0.12 < share["host"] < 0.28, share
    masked = np.mean([case["mask"] is not None for case in cases if case["layout"] != "plain4"])
    assert 0.4 < masked < 0.6
    for case in cases:
        frame = case["frame"]
        assert frame.dtype == (np.float32 if case["float"] else np.uint16) and frame.flags["C_CONTIGUOUS"]
        assert frame.ndim == 3 and frame.shape[2] == case["channels"] == stress_parity.LAYOUT_CHANNELS[case["layout"]]
        assert min(frame.shape) >= 1
        if case["mask"] is not None:
            letters = stress_parity.MASK_LETTERS[case["channels"]]
            kept = [c for c in range(case["channels"]) if c not in case["copy"]]
            assert kept and case["mask"] == "".join(letters[c] for c in kept)
            assert case["bits"] == sum(stress_parity.MASK_BITS[letter] for letter in case["mask"])
        else:
            assert case["copy"] == () and case["bits"] is None
        assert case["layout"] != "plain4" or case["mask"] is None
    if op not in (22, 25):                               # (CLAHE frames start at 16 x 16; family 25 has its own 1 x N share)
        thin = np.mean([min(case["frame"].shape[:2]) <= 3 for case in cases])
        assert 0.12 < thin < 0.4, thin


def test_statistic_windows_fit_the_lds_and_reach_every_route():
    text = source("statistic.hip")
    assert constant(text, "kStatBlock") == "kWindowBlock"
    block = int(constant(source("layout_dispatch.hpp"), "kWindowBlock"))
    most = int(constant(text, "kStatMaxLds"))
    launch = function_body(text, "MhStatus launch_statistic(")
    assert "const size_t element=rank ? 2u : (src.quantum == MH_QUANTUM_U16 ? 2u : 4u);" in launch
    assert "((W+kStatBlock-1)*(H+kStatBlock-1)*element > kStatMaxLds)" in launch
    m = re.search(r"rank \? \(n <= (\d+) \? SR_NET16 : \(n <= (\d+) \? SR_NET32 : SR_SELECT\)\)", launch)
    assert m, "the rank routes are chosen differently"
    first, second = int(m.group(1)), int(m.group(2))
    cases = draws(19)
    assert {case["args"][0] for case in cases} == set(statistic_oracle.TYPES)

    def cells(case):
        return max(case["args"][1], 1) * max(case["args"][2], 1)

    for case in cases:
        statistic, width, height = case["args"]
        element = 2 if statistic in statistic_oracle.RANK or not case["float"] else 4
        assert (max(width, 1) + block - 1) * (max(height, 1) + block - 1) * element <= most, case["args"]
        assert case["frame"].shape[0] <= 120 and case["frame"].shape[1] <= 160
    early = [cells(case) for case in cases[:FIRST] if case["args"][0] in statistic_oracle.RANK]
    assert {first - 1, first, first + 1, second - 1, second, second + 1} <= set(early), sorted(set(early))
    assert any(n <= first for n in early) and any(first < n <= second for n in early) and any(n > second for n in early)
    sides = [side for case in cases for side in case["args"][1:]]
    assert 0 in sides and any(13 <= side <= 40 for side in sides) and any(side > 40 for side in sides)
    assert any(case["args"][1] > case["frame"].shape[1] or case["args"][2] > case["frame"].shape[0] for case in cases)
    rank = [case for case in cases if case["args"][0] in statistic_oracle.RANK]
    assert 0.2 < np.mean([case["source"].startswith("repeated_keys") for case in rank]) < 0.45
    floats = [case for case in cases if case["float"] and not case["source"].startswith("repeated_keys")]
    assert np.mean([np.isnan(case["frame"]).any() for case in floats if case["frame"].size >= 1000]) > 0.9
    assert any((case["frame"] < 0).any() and (case["frame"] > 65535).any() for case in floats)


def test_edge_blur_windows_and_frames_stay_in_the_domain():
    text = source("edge_blur.hip")
    launch = function_body(text, "MhStatus launch_bilateral_blur(")
    assert "if (((W & 1u) == 0) || ((H & 1u) == 0))" in launch
    # (the header's own figures: RGBA float Quantum fits 69 x 69 bilateral and 49 x 49 selective windows)
    assert "fits square windows up to 69 x 69 (bilateral) and 49 x 49 (selective)" in " ".join(text[:4000].replace("//", " ").split())
    cases = draws(20)
    thresholds = set()
    for case in cases:
        assert case["frame"].shape[0] <= 100 and case["frame"].shape[1] <= 140
        if case["name"] == "bilateral_blur":
            width, height, intensity_sigma, spatial_sigma = case["args"]
            assert max(width, 1) % 2 == 1 and max(height, 1) % 2 == 1 and max(width, height) <= 33
            assert 1.0 <= intensity_sigma <= 250.0 and 0.5 <= spatial_sigma <= 12.0
            assert case["frame"].min() >= 300                # edge_blur_oracle: no intensity byte is 0
            assert case["intensity"] is None and case["colorspace"] == "sRGB"
        else:
            radius, sigma, threshold = case["args"]
            # at most 13 taps from the radius; from the sigma at most what test_gpu_edge_blur.py runs (0 x 4: 33 taps)
            assert (radius == 0.0 or 1.0 <= radius <= 6.0) and 0.5 <= sigma <= 4.0
            assert threshold in (0.0, 1e9) or 1.0 <= threshold <= 1e5
            thresholds.add(threshold if threshold in (0.0, 1e9) else 1.0)
            assert case["channels"] >= 3 or (case["intensity"] is None and case["colorspace"] == "sRGB")
    assert thresholds == {0.0, 1.0, 1e9}
    selective = [case for case in cases if case["name"] == "selective_blur"]
    assert {case["intensity"] for case in selective} == set(stress_parity.SELECTIVE_INTENSITIES)
    assert {case["colorspace"] for case in selective} == {"sRGB", "RGB"}
    assert 0.35 < np.mean([case["source"] == "smooth" for case in selective]) < 0.65
    assert any(case["kind"] == 5 and case["channels"] in (2, 4) for case in selective)
    bilateral = [case for case in cases if case["name"] == "bilateral_blur"]
    assert any(0 in case["args"][:2] for case in bilateral) and any(max(case["args"][:2]) > 15 for case in bilateral)
    assert any(case["float"] and case["frame"].max() > 65535 for case in bilateral)


def test_kuwahara_radii_and_layouts():
    # the first radius the library declines (test_gpu_kuwahara.py: 27 on float Quantum RGBA, 34 on Q16) is far above the draws
    cases = draws(21)
    radii = {case["args"][0] for case in cases}
    assert set(float(r) for r in stress_parity.KUWAHARA_RADII) <= radii and max(radii) <= 15.0 and any(r > 7.0 for r in radii)
    for case in cases:
        assert 0.3 <= case["args"][1] <= 3.5 and case["frame"].shape[0] <= 100 and case["frame"].shape[1] <= 140
    alpha = [case for case in cases if case["layout"] in ("gray+alpha", "rgba")]
    assert 0.2 < np.mean(["sprite_alpha" in case["source"] for case in alpha]) < 0.45
    floats = [case for case in cases if case["float"]]
    assert any("wide_range_float" in case["source"] for case in floats) and any("out_of_range_float" in case["source"] for case in floats)


def test_clahe_cases_are_ones_the_library_takes():
    text = source("clahe.hip")
    most_bins = int(constant(text, "kClaheMaxBins"))
    plan = function_body(text, "static MhStatus clahe_plan(")
    assert "const size_t bins=number_bins == 0 ? 128 : std::min<size_t>(number_bins,kClaheMaxBins);" in plan
    assert "if ((*tiles)*bins*sizeof(uint16_t) > img.bytes())" in plan
    assert "const size_t tw=width == 0 ? img.columns >> 3 : width,th=height == 0 ? img.rows >> 3 : height;" in plan
    cases = draws(22)
    for case in cases:
        width, height, number_bins, clip = case["args"]
        rows, cols, channels = case["frame"].shape
        assert 16 <= rows <= 200 and 16 <= cols <= 260 and channels in (3, 4)
        tw, th = width or cols >> 3, height or rows >> 3
        assert tw >= 1 and th >= 1 and number_bins != 1 and clip >= 0.0
        bins = 128 if number_bins == 0 else min(number_bins, most_bins)
        tiles = ((cols + tw - 1) // tw) * ((rows + th - 1) // th)
        assert tiles * bins * 2 <= case["frame"].nbytes
        assert clahe_oracle.table_fits(rows, cols, channels, case["frame"].dtype, width, height, number_bins)
        assert case["colorspace"] == "Lab" or not case["float"]
    assert {case["colorspace"] for case in cases if not case["float"]} == {"sRGB", "Lab"}
    assert {case["args"][2] for case in cases} == set(stress_parity.CLAHE_BINS)
    assert set(stress_parity.CLAHE_CLIPS) <= {case["args"][3] for case in cases}
    assert 0 in {case["args"][0] for case in cases} and 0 in {case["args"][1] for case in cases}
    assert any("float_specials" in case["source"] for case in cases)


def test_threshold_cases_stay_off_what_the_library_declines():
    span, band_rows, most_width, most_float_side = adaptive_constants()
    assert (span, band_rows, most_width) == (stress_parity.ADAPTIVE_SPAN, stress_parity.ADAPTIVE_BAND_ROWS,
                                             stress_parity.ADAPTIVE_MAX_WIDTH)
    gray = function_body(source("operators_enhance.cpp"), "static bool threshold_gray_frame(")
    assert "MH_COLORSPACE_GRAY" in gray and "colours" in gray
    cases = draws(23)
    counts = {name: sum(case["name"] == name for case in cases) for name in stress_parity.THRESHOLD_OPERATORS}
    assert max(counts.values()) - min(counts.values()) <= 1, counts

    def over_a_strip(case):
        return not case["float"] and case["frame"].shape[1] > span - (max(case["args"][0], 1) - 1)

    def over_a_band(case):
        return not case["float"] and case["frame"].shape[0] > max(band_rows, 4 * case["args"][1])

    for case in cases:
        name, rows, cols = case["name"], case["frame"].shape[0], case["frame"].shape[1]
        if name in ("black", "white", "range"):
            assert case["layout"] in ("rgb", "rgba", "plain4") and case["colorspace"] in ("sRGB", "RGB")
        if name == "adaptive":
            width, height, bias = case["args"]
            assert width <= (most_float_side if case["float"] else most_width) and height <= 150
            assert case["float"] or height <= 65537
            if case["shape"] == "plain":
                assert rows <= 140 and cols <= 200
        else:
            assert rows <= 140 and cols <= 200
        assert case["intensity"] is None or (case["layout"] in ("rgb", "rgba") and name in ("bilevel", "auto"))
    adaptive = [case for case in cases if case["name"] == "adaptive"]
    early = [case for case in cases[:FIRST] if case["name"] == "adaptive"]
    assert any(over_a_strip(case) for case in early), "no adaptive case over one strip among the first %d" % FIRST
    assert any(over_a_band(case) for case in early), "no adaptive case over one band among the first %d" % FIRST
    assert {case["shape"] for case in adaptive} == {"plain", "strip", "band"}
    assert all(over_a_strip(case) for case in adaptive if case["shape"] == "strip")
    assert all(over_a_band(case) for case in adaptive if case["shape"] == "band")
    assert any(case["args"][0] > 40 for case in adaptive) and any(case["args"][1] > 40 for case in adaptive)
    assert any(0 in case["args"][:2] for case in adaptive)
    assert any("wide_range_float" in case["source"] for case in adaptive)
    assert {case["args"][0] for case in cases if case["name"] == "auto"} == set(threshold_oracle.METHODS)
    assert {case["intensity"] for case in cases} == set(threshold_oracle.INTENSITIES) | {None}
    # a threshold exactly on a sample of the frame, within the first cases too: the < / <= edges
    def on_a_sample(case):
        levels = case["args"][0] if case["name"] in ("black", "white") else case["args"]
        return any(np.float64(level) in case["frame"].astype(np.float64) for level in levels)
    assert any(on_a_sample(case) for case in cases[:FIRST] if case["name"] == "bilevel")
    for name in ("black", "white", "range"):
        assert any(on_a_sample(case) for case in cases if case["name"] == name)
    assert any(case["source"] == "constant" for case in cases) and any(case["source"].startswith("two_level") for case in cases)


def test_level_parameters_cover_their_ranges():
    cases = draws(24)
    # NormalizeImage is ContrastStretchImage, which declines a colour frame whose every pixel is gray
    stretch = function_body(source("operators_enhance.cpp"), "MH_API MhStatus MagickHipContrastStretchImage(")
    assert "ContrastStretchImage: image is gray" in stretch and "(colour >= 3)" in stretch
    assert any(case["kind"] == 4 and case["channels"] >= 3 for case in cases)       # the checkerboard: R == G == B everywhere
    for case in cases:
        assert case["frame"].shape[0] <= 200 and case["frame"].shape[1] <= 260
        if case["name"] == "normalize" and case["channels"] >= 3:
            p = case["frame"][..., :3].astype(np.float64)
            assert not ((np.abs(p[..., 0] - p[..., 1]) < 1.0e-12) & (np.abs(p[..., 1] - p[..., 2]) < 1.0e-12)).all()
        assert case["libm"] in (False, True)
        if case["name"] in ("gamma", "negate", "auto_level", "linear_stretch", "normalize", "brightness_contrast"):
            assert not case["libm"]                      # test_gpu_levels.py: table-driven or no libm at all
        if case["name"] == "sigmoidal":
            assert case["libm"] and 0.01 <= case["args"][1] <= 20.0 and -1000.0 <= case["args"][2] <= 70000.0
        if case["name"] == "linear_stretch":
            pixels = case["frame"].shape[0] * case["frame"].shape[1]
            assert 0.0 <= case["args"][0] <= pixels and 0.0 <= case["args"][1] <= pixels
    levels = [case for case in cases if case["name"] in ("level", "levelize")]
    assert any(case["args"][1] < case["args"][0] for case in levels) and any(case["args"][0] < 0 for case in levels)
    gammas = {case["args"][2] for case in levels} | {case["args"][0] for case in cases if case["name"] == "gamma"}
    assert {0.0, 1.0} <= gammas and any(0.1 <= g < 1.0 for g in gammas) and any(1.0 < g <= 10.0 for g in gammas)
    assert all(g in (0.0, 1.0) or 0.1 <= g <= 10.0 for g in gammas)
    assert {case["args"][0] for case in cases if case["name"] in ("negate", "sigmoidal")} == {False, True}
    colour = [case for case in cases if case["channels"] >= 3]
    assert 0.15 < np.mean(["gray_pixels" in case["source"] for case in colour]) < 0.35
    assert {case["libm"] for case in levels} == {False, True}


def test_scale_geometries():
    cases = draws(25)

    def kind(case):
        (rows, cols), (to_rows, to_cols) = case["frame"].shape[:2], case["args"]
        if (to_rows, to_cols) == (rows, cols):
            return "identity"
        if to_rows >= rows and to_cols >= cols:
            return "enlargement"
        if to_rows <= rows and to_cols <= cols:
            return "reduction"
        return "mixed"

    assert {"enlargement", "reduction", "mixed"} <= {kind(case) for case in cases[:FIRST]}
    for case in cases:
        (rows, cols), (to_rows, to_cols) = case["frame"].shape[:2], case["args"]
        assert 1 <= rows <= 300 and 1 <= cols <= 300 and 1 <= to_rows <= 400 and 1 <= to_cols <= 400
        assert case["name"] != "thumbnail" or case["layout"] in ("rgb", "rgba")
        assert (case["offset"] is None) or case["name"] == "sample"
        if case["name"] == "sample" and kind(case) != "identity":
            ox, oy = scale_oracle.offset_percent(case["offset"])
            assert scale_oracle.sample_offsets(rows, to_rows, oy).max() < rows
            assert scale_oracle.sample_offsets(cols, to_cols, ox).max() < cols
    assert {case["offset"] for case in cases if case["name"] == "sample"} == set(scale_oracle.SAMPLE_OFFSETS)
    assert 0.1 < np.mean([min(case["frame"].shape[:2]) == 1 for case in cases]) < 0.3

    def whole_factor(case):
        (rows, cols), (to_rows, to_cols) = case["frame"].shape[:2], case["args"]
        return kind(case) != "identity" and ((to_rows % rows == 0 and to_cols % cols == 0) or (rows % to_rows == 0 and cols % to_cols == 0))

    def coprime(case):
        (rows, cols), (to_rows, to_cols) = case["frame"].shape[:2], case["args"]
        return np.gcd(rows, to_rows) == 1 and np.gcd(cols, to_cols) == 1

    assert np.mean([whole_factor(case) for case in cases]) > 0.07 and np.mean([coprime(case) for case in cases]) > 0.1
    alpha = [case for case in cases if case["layout"] in ("gray+alpha", "rgba")]
    assert {"transparent 0", "transparent 0.2", "transparent 0.9"} <= {case["source"].split(" ", 3)[3] for case in alpha
                                                                        if case["source"].startswith("frame")}
    assert any(case["source"].startswith("negative_alpha_float") for case in alpha)
    assert not any(case["source"].startswith("negative_alpha_float") for case in cases if case["layout"] in ("gray", "rgb"))
