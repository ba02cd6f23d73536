"""How long every work item of the hybrid FAST blur's ONE launch takes (diagnostic build -DMH_HYBRID_ITEMS of
convolve_fused_hybrid.hip): lane 0 of wave 0 of every workgroup stamps the shader clock and the constant-rate
clock when it starts and when it has left the walk.  The launch is one round of one workgroup a CU, so it lasts
as long as its slowest item; the items of the first and the last strip stage a window that hangs over the image.

  build:  make -C imagemagick_amd/csrc VARIANT=items VDEFS=-DMH_HYBRID_ITEMS VFILES=convolve_fused_hybrid.hip
  run:    MAGICKHIP_LIBRARY=$PWD/imagemagick_amd/lib/libmagickhip_items.so python tools/hybrid_item_balance.py [rgba|plain|rgb] [size] [launches]

Prints a markdown table: per launch the interior items' median / maximum and every edge item, in shader-clock
cycles and in microseconds of the constant-rate clock (100 MHz), and who ended last.
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MAGICKHIP_HYBRID_ITEMS", "/tmp/hybrid_items.bin")
import numpy as np
import torch
import imagemagick_amd as im

layout = sys.argv[1] if len(sys.argv) > 1 else "rgba"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
launches = int(sys.argv[3]) if len(sys.argv) > 3 else 5
TICK_US = 0.01      # the constant-rate clock: 100 MHz

im.load()
im.set_option("MAGICKHIP_HYBRID_ITEMS", os.environ["MAGICKHIP_HYBRID_ITEMS"])     # (a selector switch: not read from the environment)
im.set_precision(im.PRECISION_FAST)
torch.manual_seed(5)
channels = 3 if layout == "rgb" else 4
a = torch.randint(-32768, 32768, (n, n, channels), device="cuda", dtype=torch.int16).view(torch.uint16)
img = im.Image(a, has_alpha=layout == "rgba")
for _ in range(3):
    im.blur_image(img, 0.0, 10.0)
torch.cuda.synchronize()


def name(item, strips):
    return "strip %d segment %d" % (item % strips, item // strips)


print("%s %dx%d, BlurImage(0, 10), library %s" % (layout, n, n, os.path.basename(im._lib.LIB_PATH)))
print()
print("| launch | interior median (cycles) | interior max | interior p5..p95 | edge items (cycles) | edge/median | "
      "interior median (us) | edge (us) | launch span (us) | last to end |")
print("|---|---|---|---|---|---|---|---|---|---|")
ratios, medians = [], []
for launch in range(launches):
    im.blur_image(img, 0.0, 10.0)
    torch.cuda.synchronize()
    raw = np.fromfile(os.environ["MAGICKHIP_HYBRID_ITEMS"], dtype=np.uint64).astype(np.int64)
    strips, segments = int(raw[0]), int(raw[1])
    t = raw[2:].reshape(strips * segments, 4)
    cycles, ticks = t[:, 1] - t[:, 0], (t[:, 3] - t[:, 2]) * TICK_US
    edge = np.array([(i % strips) in (0, strips - 1) for i in range(strips * segments)])
    inner_c, inner_t = cycles[~edge], ticks[~edge]
    median = float(np.median(inner_c))
    span = (t[:, 3].max() - t[:, 2].min()) * TICK_US
    last = int(np.argmax(t[:, 3]))
    ratios.append(float(cycles[edge].mean()) / median)
    medians.append(median)
    print("| %d | %.0f | %.0f | %.0f..%.0f | %s | %s | %.1f | %s | %.1f | %s |" % (
        launch, median, inner_c.max(), np.percentile(inner_c, 5), np.percentile(inner_c, 95),
        ", ".join("%s: %d" % (name(i, strips), cycles[i]) for i in np.flatnonzero(edge)),
        ", ".join("%.3f" % (cycles[i] / median) for i in np.flatnonzero(edge)),
        float(np.median(inner_t)), ", ".join("%.1f" % ticks[i] for i in np.flatnonzero(edge)), span, name(last, strips)))
print()
print("edge items against the interior median, mean over the launches: %.3f; interior median %.0f cycles "
      "(spread over the launches %.0f..%.0f)" % (float(np.mean(ratios)), float(np.median(medians)), min(medians), max(medians)))
