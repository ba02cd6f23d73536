"""The change-count restatement of tests/morphology_oracle.py against counts worked out by hand (no GPU, no
compiled reference): the GPU tests of test_gpu_morphology_count.py compare the library with it."""
import numpy as np

from morphology_oracle import changed_count, unrounded

IDENTITY = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
BINOMIAL = np.array([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]])


def test_identity_kernel_counts_through_the_bias_alone():
    """0,0,0 0,1,0 0,0,0: the sum is the sample itself.  Without a bias nothing changes; a bias of a quarter of a
    level changes every unrounded value (and no rounded one)."""
    px = np.arange(12, dtype=np.uint16).reshape(3, 4, 1) * 5000
    assert changed_count(px, "Convolve", IDENTITY, 1, 1, 0.0) == (0, 0)
    assert changed_count(px, "Convolve", IDENTITY, 1, 1, 0.25) == (12, 12)
    assert np.array_equal(unrounded(px, "Convolve", IDENTITY, 1, 1, 0.25), px + 0.25)


def test_clamped_sums_count_although_the_level_stays():
    """1,2,1 2,4,2 1,2,1 unnormalised over one row 0 0 0 65535 65535 (the rows above and below are its edge copies:
    a factor of 4 on the row kernel 1,2,1).  Sums: 0, 0, 4*65535, 4*3*65535, 4*4*65535 — the last two clamp back to
    the source level 65535 and count all the same; the two zeros do not."""
    px = np.array([[0, 0, 0, 65535, 65535]], dtype=np.uint16).reshape(1, 5, 1)
    sums = unrounded(px, "Convolve", BINOMIAL, 1, 1)[0, :, 0]
    assert sums.tolist() == [0.0, 0.0, 262140.0, 786420.0, 1048560.0]
    assert changed_count(px, "Convolve", BINOMIAL, 1, 1) == (3, 3)
    # a bias that cancels the first changed sum exactly: one sample fewer ... and two more where the sum was 0
    assert changed_count(px, "Convolve", BINOMIAL, 1, 1, -262140.0) == (4, 4)


def test_convolve_reflects_the_kernel_about_its_origin():
    """2x1+0+0: a,b gives b*p[x-1] + a*p[x] (morphology.c:2623, :2938): `0,1` moves the row one sample to the
    right, `1,0` leaves it alone."""
    px = np.array([[1, 2, 2, 5]], dtype=np.uint16).reshape(1, 4, 1)
    assert unrounded(px, "Convolve", [[0.0, 1.0]], 0, 0)[0, :, 0].tolist() == [1.0, 1.0, 2.0, 2.0]
    assert changed_count(px, "Convolve", [[0.0, 1.0]], 0, 0) == (2, 2)
    assert changed_count(px, "Convolve", [[1.0, 0.0]], 0, 0) == (0, 0)
    # Erode takes the kernel as it stands, Dilate reflected: with the origin at the left cell Erode looks right
    assert unrounded(px, "Erode", [[1.0, 1.0]], 0, 0)[0, :, 0].tolist() == [1.0, 2.0, 2.0, 5.0]
    assert unrounded(px, "Dilate", [[1.0, 1.0]], 0, 0)[0, :, 0].tolist() == [1.0, 2.0, 2.0, 5.0]
    assert unrounded(px[:, ::-1], "Erode", [[1.0, 1.0]], 0, 0)[0, :, 0].tolist() == [2.0, 2.0, 1.0, 1.0]
    assert unrounded(px[:, ::-1], "Dilate", [[1.0, 1.0]], 0, 0)[0, :, 0].tolist() == [5.0, 5.0, 2.0, 2.0]


def test_erode_and_dilate_counts_nan_cells_and_the_channel_divisor():
    """Row 5 3 9 9 under 1,1,1: Erode 3 3 3 9 (two samples change), Dilate 5 9 9 9 (one); a NaN cell is no part
    of the kernel.  Three channels of which one is masked: it does not count, and the count is divided by the two
    that carry the update trait (GetImageChannels)."""
    row = np.array([[5, 3, 9, 9]], dtype=np.uint16).reshape(1, 4, 1)
    ones = [[1.0, 1.0, 1.0]]
    assert changed_count(row, "Erode", ones, 1, 0) == (2, 2)
    assert changed_count(row, "Dilate", ones, 1, 0) == (1, 1)
    assert changed_count(row, "Erode", [[np.nan, 1.0, 1.0]], 1, 0) == (1, 1)          # 3 3 9 9
    assert changed_count(row, "Dilate", [[np.nan, 1.0, 1.0]], 1, 0) == (1, 1)         # reflected, looks left: 5 5 9 9
    px = np.repeat(row, 3, axis=2)
    px[0, :, 1] = (7, 7, 7, 1)
    assert changed_count(px, "Erode", ones, 1, 0) == (5, 1)                             # 2 + 1 + 2 samples over 3
    assert changed_count(px, "Erode", ones, 1, 0, copy_channels=(1,)) == (4, 2)
    assert changed_count(px, "Convolve", IDENTITY, 1, 1, 0.25, copy_channels=(1,)) == (8, 4)


def test_restated_pixels_are_the_compiled_references(refmod):
    """The restatement's `pixel`, clamped and rounded as ClampToQuantum does, is what the compiled reference stores
    — on the frames and kernels the GPU tests count on."""
    from test_gpu_morphology_count import frame, CONVOLVE_CASES, MINMAX_KERNELS
    cases = [("Convolve", k, b) for k, b in CONVOLVE_CASES] + [(m, k, 0.0) for m in ("Erode", "Dilate") for k in MINMAX_KERNELS]
    for channels in (1, 3):
        px = frame(channels, np.uint16)
        for method, kernel, bias in cases:
            values, x, y, _ = refmod.kernel(kernel)
            ref = refmod.RefImage(px)
            if bias != 0.0:
                ref.set_artifact("convolve:bias", "%.17g" % bias)
            want = ref.morphology(method, 1, kernel).numpy().reshape(px.shape)
            pixel = unrounded(px, method, values, x, y, bias)
            got = np.floor(np.clip(pixel, 0.0, 65535.0) + 0.5).astype(np.uint16)
            assert np.array_equal(got, want), "%s %s bias %g, %d channels" % (method, kernel, bias, channels)
