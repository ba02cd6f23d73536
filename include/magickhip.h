/*
  magickhip.h — C ABI of libmagickhip.so, an MI355X (gfx950 / CDNA4) native
  accelerate backend for MagickCore.

  This is the drop-in boundary: plain C, plain pointers and sizes, no C++ or
  torch types.  Every operator entry point below replaces (or adds, where the
  reference has no hook) one `Accelerate*Image()` function of the reference:

    reference interface                           file:line
    --------------------------------------------  -----------------------------------
    AccelerateBlurImage                           MagickCore/accelerate-private.h:36-37
    AccelerateResizeImage                         MagickCore/accelerate-private.h:43-44
    AccelerateUnsharpMaskImage                    MagickCore/accelerate-private.h:46-47
    AccelerateContrastStretchImage                MagickCore/accelerate-private.h:52-53
    AccelerateEqualizeImage                       MagickCore/accelerate-private.h:54
    AccelerateFunctionImage                       MagickCore/accelerate-private.h:56-57
    AccelerateGrayscaleImage                      MagickCore/accelerate-private.h:58-59
    (new) convolve / morphology hook              MagickCore/morphology.c:3937, :4219
    (new) colourspace hook                        MagickCore/colorspace.c:1751
    checkAccelerateCondition (the gate)           MagickCore/accelerate.c:110-170
    SetOpenCLEnabled / GetOpenCLEnabled           MagickCore/opencl.h, opencl.c:3192
    GetOpenCLKernelProfileRecords                 MagickCore/opencl.c:2081
    KernelInfo                                    MagickCore/morphology.h:100-127
    MorphologyMethod                              MagickCore/morphology.h:72-98
    PixelTrait                                    MagickCore/pixel.h:146-152
    FilterType                                    MagickCore/resample.h:31-69

  Conventions (same as the reference's accelerate layer):
    * every operator returns MH_OK (0) when it produced the result, and a
      non-zero MhStatus when it did not — the caller then runs its CPU path,
      exactly as it does when Accelerate*Image() returns NULL / MagickFalse
      (MagickCore/effect.c:783-787).  Nothing here throws or aborts.
    * the caller owns every pixel buffer; the library owns device memory,
      streams and staging buffers.
    * pixel layout is the pixel cache's: row-major, channel-interleaved
      Quantum[rows][columns][number_channels] (MagickCore/cache-private.h:130-226,
      MagickCore/pixel.c:6132-6205).  Quantum is `unsigned short` (Q16) or
      `float` (Q16-HDRI) — MagickCore/magick-type.h:80-88.
    * results are those of the reference CPU path: see DESIGN.md "Parity".
*/
#ifndef MAGICKHIP_H
#define MAGICKHIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(__cplusplus)
extern "C" {
#endif

#if defined(MAGICKHIP_BUILD)
#  define MH_API __attribute__((visibility("default")))
#else
#  define MH_API
#endif

#define MH_MAX_CHANNELS 4   /* the accelerate gate admits R[,G,B][,A] only: accelerate.c:142-167 */

typedef enum
{
  MH_OK = 0,
  MH_UNSUPPORTED = 1,     /* gate failed: caller should use the CPU path */
  MH_NO_DEVICE = 2,
  MH_BAD_ARGUMENT = 3,
  MH_OUT_OF_MEMORY = 4,
  MH_DEVICE_ERROR = 5,
  MH_DISABLED = 6         /* MhSetEnabled(0) or MAGICK_HIP_DEVICE=off */
} MhStatus;

typedef enum
{
  MH_QUANTUM_U16 = 0,     /* Q16:      Quantum = unsigned short */
  MH_QUANTUM_F32 = 1      /* Q16-HDRI: Quantum = float, nominal range 0..65535 */
} MhQuantumKind;

typedef enum
{
  MH_MEMORY_HOST = 0,     /* pixels is a host pointer (e.g. CacheInfo::pixels); staged with hipMemcpyAsync */
  MH_MEMORY_DEVICE = 1    /* pixels is a device pointer on `device`; used in place */
} MhMemoryKind;

/* PixelTrait bits, MagickCore/pixel.h:146-152 */
enum
{
  MH_TRAIT_UNDEFINED = 0x0,
  MH_TRAIT_COPY = 0x1,
  MH_TRAIT_UPDATE = 0x2,
  MH_TRAIT_BLEND = 0x4
};

/* ColorspaceType, MagickCore/colorspace.h:25-67 (same values).  TransformImageColorspace is
   accelerated between sRGB and every pointwise colourspace of ConvertRGBToGeneric /
   ConvertGenericToRGB (colorspace.c:411-595, :122-305) plus linear RGB; GRAY / LinearGRAY only
   describe single-channel images; CMYK, Log, OHTA, Rec601/709YCbCr, scRGB, YCC, Transparent
   stay on the CPU path. */
typedef enum
{
  MH_COLORSPACE_UNDEFINED = 0,
  MH_COLORSPACE_CMY = 1,
  MH_COLORSPACE_GRAY = 3,
  MH_COLORSPACE_HCL = 4,
  MH_COLORSPACE_HCLP = 5,
  MH_COLORSPACE_HSB = 6,
  MH_COLORSPACE_HSI = 7,
  MH_COLORSPACE_HSL = 8,
  MH_COLORSPACE_HSV = 9,
  MH_COLORSPACE_HWB = 10,
  MH_COLORSPACE_LAB = 11,
  MH_COLORSPACE_LCH = 12,      /* alias of LCHab in the pixel loops (colorspace.c:488-489) */
  MH_COLORSPACE_LCHAB = 13,
  MH_COLORSPACE_LCHUV = 14,
  MH_COLORSPACE_LOG = 15,          /* default film parameters only (colorspace.c:1057-1060) */
  MH_COLORSPACE_LMS = 16,
  MH_COLORSPACE_LUV = 17,
  MH_COLORSPACE_OHTA = 18,         /* the table-driven transforms, colorspace.c:1254-1420, :2591-2790 */
  MH_COLORSPACE_REC601YCBCR = 19,
  MH_COLORSPACE_REC709YCBCR = 20,
  MH_COLORSPACE_RGB = 21,      /* linear RGB */
  MH_COLORSPACE_SCRGB = 22,        /* the same pixel loops as RGB (colorspace.c:1164-1165, :2502-2503) */
  MH_COLORSPACE_SRGB = 23,
  MH_COLORSPACE_XYY = 25,
  MH_COLORSPACE_XYZ = 26,
  MH_COLORSPACE_YCBCR = 27,
  MH_COLORSPACE_YCC = 28,          /* as a target only: YCC -> sRGB (YCCMap) is declined */
  MH_COLORSPACE_YDBDR = 29,
  MH_COLORSPACE_YIQ = 30,
  MH_COLORSPACE_YPBPR = 31,
  MH_COLORSPACE_YUV = 32,
  MH_COLORSPACE_LINEARGRAY = 33,
  MH_COLORSPACE_JZAZBZ = 34,
  MH_COLORSPACE_DISPLAYP3 = 35,
  MH_COLORSPACE_ADOBE98 = 36,
  MH_COLORSPACE_PROPHOTO = 37,
  MH_COLORSPACE_OKLAB = 38,
  MH_COLORSPACE_OKLCH = 39,
  MH_COLORSPACE_CAT02LMS = 40
} MhColorspace;

/* PixelIntensityMethod, MagickCore/pixel.h */
typedef enum
{
  MH_INTENSITY_UNDEFINED = 0,
  MH_INTENSITY_AVERAGE = 1,
  MH_INTENSITY_BRIGHTNESS = 2,
  MH_INTENSITY_LIGHTNESS = 3,
  MH_INTENSITY_MS = 4,
  MH_INTENSITY_REC601LUMA = 5,
  MH_INTENSITY_REC601LUMINANCE = 6,
  MH_INTENSITY_REC709LUMA = 7,
  MH_INTENSITY_REC709LUMINANCE = 8,
  MH_INTENSITY_RMS = 9
} MhIntensityMethod;

/* ChannelType bits that change operator behaviour, MagickCore/pixel.h:60-75 */
#define MH_ALL_CHANNELS 0x7FFFFFFu
#define MH_SYNC_CHANNELS 0x20000u

/*
  One image as the operators see it: what the shim extracts from `Image` /
  `CacheInfo` (SURVEY §8b "Data access").
*/
typedef struct MhImage
{
  void *pixels;
  size_t columns;
  size_t rows;
  uint32_t number_channels;                 /* 1..MH_MAX_CHANNELS */
  uint32_t quantum;                         /* MhQuantumKind */
  uint32_t memory;                          /* MhMemoryKind */
  int32_t device;                           /* HIP device ordinal; -1 = library default; MH_DEVICE_ALL (host memory,
                                               new-image stencil operators on frames of 64 MB and more): the row
                                               bands of the frame go round every (logical) device of the node */
  uint32_t channel_traits[MH_MAX_CHANNELS]; /* PixelTrait of the channel stored at each offset */
  int32_t alpha_offset;                     /* offset of the alpha channel, -1 if none (image->alpha_trait undefined) */
  uint32_t alpha_trait;                     /* image->alpha_trait: MH_TRAIT_BLEND when alpha is active */
  uint32_t colorspace;                      /* MhColorspace */
  uint32_t intensity;                       /* MhIntensityMethod; 0 = default (Rec709Luma) */
  uint32_t channel_mask;                    /* image->channel_mask (ChannelType bits); MH_ALL_CHANNELS by default */
  void *stream;                             /* hipStream_t to run on; NULL = library stream.  DEVICE images only */
  uint32_t precision;                       /* 0 = the library default (MhSetPrecision); else MhPrecision + 1:
                                               the precision of THIS call, whatever other threads run with */
} MhImage;

/* Fill the traits the way InitializePixelChannelMap does for an image with
   `number_channels` channels and optional alpha (pixel.c:6132-6205,
   SetPixelChannelMask pixel.c:6338-6393 with the default channel mask). */
MH_API void MhInitImage(MhImage *image,void *pixels,size_t columns,size_t rows,
  uint32_t number_channels,int has_alpha,MhQuantumKind quantum,
  MhMemoryKind memory);

/* ------------------------------------------------------------------ runtime */

MH_API MhStatus MhInitialize(void);               /* InitializeOpenCL analogue, opencl.c:2430 */
MH_API void MhTerminus(void);                     /* OpenCLTerminus, opencl.c:2576 */
MH_API int MhDeviceCount(void);
#define MH_DEVICE_ALL (-2)
MH_API MhStatus MhSetDevice(int device);          /* default device for device=-1 images */
/* bands the host-image pipeline (MH_DEVICE_ALL included) has finished on a logical device: tests, bench */
MH_API unsigned long long MhBandedBands(int logical_device);
MH_API int MhGetEnabled(void);                    /* GetOpenCLEnabled */
MH_API int MhSetEnabled(int enabled);             /* SetOpenCLEnabled, opencl.c:3192; returns new state */
MH_API const char *MhGetLastError(void);          /* thread-local description of the last non-OK status */
MH_API const char *MhGetVersion(void);

typedef enum
{
  MH_PRECISION_EXACT = 0,  /* FP64, the CPU's operation order, no FMA contraction: bit-identical results */
  MH_PRECISION_FAST = 1    /* FP32 FMA accumulation where the result is still within +-1 Quantum level (Q16 only) */
} MhPrecision;
/* The library-wide DEFAULT: MH_PRECISION_FAST — what an unchanged MagickCore caller gets through the
   shim, within the +-1 level / +-1 ULP the drop-in promises (the reference's own OpenCL path computes
   in float and is not bit-identical to its CPU path either); MAGICK_HIP_PRECISION=exact at start-up
   or MhSetPrecision(MH_PRECISION_EXACT) selects the bit-identical mode.  A call whose first image
   carries a non-zero MhImage::precision runs with that precision instead: two threads can run
   EXACT and FAST operators at the same time. */
MH_API MhPrecision MhGetPrecision(void);
MH_API MhPrecision MhSetPrecision(MhPrecision precision);
#define MH_IMAGE_PRECISION(p) ((uint32_t) (p)+1u)      /* value for MhImage::precision */

/* Options.  Every MAGICKHIP_* / MAGICK_HIP_* environment variable is read ONCE, when the runtime
   initialises (MhInitialize or the first call); later changes of the environment are not seen.
   MhSetOption changes the value the library holds (value == NULL: as if the variable were unset)
   — for tests and A/B measurements; MhGetOption returns it (NULL when unset; the pointer stays
   valid).  Names as documented in DESIGN.md, e.g. "MAGICKHIP_NO_MFMA". */
MH_API MhStatus MhSetOption(const char *name,const char *value);
MH_API const char *MhGetOption(const char *name);

/* What the device arbitration of the MagickCore binding needs (the reference: RequestOpenCLDevice,
   opencl.c:3056-3102; AcquireOpenCLCommandQueue, opencl.c:656; GetOpenCLDevices and the device
   getters, opencl.c:1823-2130).  `device` is a HIP ordinal below MhDeviceCount().
   MhLogicalDeviceCount: the number of devices a caller should arbitrate over — MhDeviceCount(),
   or MAGICKHIP_LOGICAL_DEVICES when that is larger (logical device d runs on physical device
   d mod MhDeviceCount(): how a one-GPU box rehearses the multi-GPU paths). */
typedef struct MhDeviceInfo
{
  char name[128];            /* e.g. "AMD Instinct MI355X" */
  char architecture[64];     /* e.g. "gfx950:sramecc+:xnack-" */
  int32_t compute_units;
  int32_t clock_mhz;
  uint64_t global_memory;    /* bytes */
  uint64_t local_memory;     /* LDS bytes per workgroup */
} MhDeviceInfo;
MH_API int MhLogicalDeviceCount(void);
MH_API MhStatus MhGetDeviceInfo(int device,MhDeviceInfo *info);
/* A non-blocking stream on `device` (the caller passes it as MhImage::stream and to the transfer
   helpers); destroyed by MhStreamDestroy or MhTerminus. */
MH_API MhStatus MhStreamCreate(int device,void **stream);
MH_API MhStatus MhStreamDestroy(int device,void *stream);
/* Image-sized device blocks from the library's stream-ordered caching pool: no hipMalloc /
   hipFree (a device-wide synchronisation) per operator result.  `stream` = the stream the block
   was last used on; MhDeviceFreeAsync returns at once, and the block is handed out again only
   behind the work enqueued on that stream. */
MH_API MhStatus MhDeviceAllocAsync(int device,size_t bytes,void *stream,void **ptr);
MH_API MhStatus MhDeviceFreeAsync(int device,void *ptr,void *stream);

/* Device memory helpers for callers that keep images resident.  MhUpload returns once the
   transfer is enqueued on `stream` and `src_host` may be reused; MhDownload returns once
   `dst_host` holds the data.  Pageable host blocks of 8 MiB and more move through page-locked
   staging buffers on a few host threads (replaces opencl.c's clEnqueueMapBuffer round trips,
   MagickCore/cache.c:5341-5353). */
MH_API MhStatus MhDeviceAlloc(int device,size_t bytes,void **ptr);
MH_API MhStatus MhDeviceFree(int device,void *ptr);
MH_API MhStatus MhUpload(int device,void *dst_device,const void *src_host,size_t bytes,void *stream);
MH_API MhStatus MhDownload(int device,void *dst_host,const void *src_device,size_t bytes,void *stream);
MH_API MhStatus MhSynchronize(int device,void *stream);

/* Page-locked host memory for pixel caches (what SetMagickAlignedMemoryMethods,
   MagickCore/memory.c:1541, lets an application install behind AcquireAlignedMemory,
   cache.c:3754-3758): a host image whose `pixels` block came from MhHostAlloc moves over the
   link with one DMA transfer per direction, no staging threads.  MhHostFree returns 1 when the
   block was one of MhHostAlloc's (and is now released), 0 when it is not known (the caller then
   releases it its own way).  MhHostAllocatedBytes: the bytes currently handed out. */
MH_API void *MhHostAlloc(size_t bytes);
MH_API int MhHostFree(void *block);
MH_API size_t MhHostAllocatedBytes(void);
/* ... plus the released blocks the library keeps page-locked for reuse (MAGICKHIP_PINNED_SPARE_BYTES,
   1 GiB by default): what a budget on page-locked memory has to count */
MH_API size_t MhHostPinnedBytes(void);

/* Kernel profile records (GetOpenCLKernelProfileRecords analogue). */
typedef struct MhKernelProfileRecord
{
  const char *kernel_name;
  unsigned long count;
  double min_ms,max_ms,total_ms;   /* hipEvent-timed, only while profiling is enabled */
} MhKernelProfileRecord;
MH_API int MhSetProfileEnabled(int enabled);      /* SetOpenCLKernelProfileEnabled, opencl.c:3162 */
MH_API size_t MhGetProfileRecords(MhKernelProfileRecord *records,size_t capacity);
/* ... of one device only (GetOpenCLKernelProfileRecords(device, &length), opencl.c:2081) */
MH_API size_t MhGetDeviceProfileRecords(int device,MhKernelProfileRecord *records,size_t capacity);
MH_API void MhResetProfileRecords(void);

/* Diagnostics of the exact-integer blur (convolve_fused_exact.hip): the number of samples whose
   level the integer sums' error bound could not decide and that were recomputed in the
   reference's own operation order (morphology.c:2746-2764).  enable != 0 starts counting on the
   current device (the counter is read and reset by every call); returns the count so far. */
MH_API unsigned long long MhExactBlurRecomputed(int enable);
/* The same for the separable EXACT 2-D Convolve (GaussianBlurImage in EXACT mode and on float
   Quantum): samples recomputed in the reference's w x h order. */
MH_API unsigned long long MhSeparableRecomputed(int enable);
/* Diagnostic of the exact-integer 2-D convolve (cells that are integer multiples of a unit: every
   flat shape kernel; morphology.c:2919-2979 on the i8 matrix cores, bit-identical): samples that
   lay within the reference's own rounding error of a Quantum boundary and were recomputed in the
   reference's order since the last call (enable as above). */
MH_API unsigned long long MhConvolve2DRecomputed(int enable);
/* ... and of the fused fp64 2-D convolve that takes every other kernel and frame (one fused
   multiply-add per cell and channel over alpha-premultiplied doubles + tie check, bit-identical). */
MH_API unsigned long long MhConvolve2DTieRecomputed(int enable);


/* ------------------------------------------------------ kernels and filters */

/* KernelInfoType, MagickCore/morphology.h:30-70 (same order) */
typedef enum
{
  MH_KERNEL_UNDEFINED = 0,
  MH_KERNEL_UNITY, MH_KERNEL_GAUSSIAN, MH_KERNEL_DOG, MH_KERNEL_LOG, MH_KERNEL_BLUR,
  MH_KERNEL_COMET, MH_KERNEL_BINOMIAL, MH_KERNEL_LAPLACIAN, MH_KERNEL_SOBEL,
  MH_KERNEL_FREICHEN, MH_KERNEL_ROBERTS, MH_KERNEL_PREWITT, MH_KERNEL_COMPASS,
  MH_KERNEL_KIRSCH, MH_KERNEL_DIAMOND, MH_KERNEL_SQUARE, MH_KERNEL_RECTANGLE,
  MH_KERNEL_OCTAGON, MH_KERNEL_DISK, MH_KERNEL_PLUS, MH_KERNEL_CROSS, MH_KERNEL_RING,
  MH_KERNEL_PEAKS, MH_KERNEL_EDGES, MH_KERNEL_CORNERS, MH_KERNEL_DIAGONALS,
  MH_KERNEL_LINEENDS, MH_KERNEL_LINEJUNCTIONS, MH_KERNEL_RIDGES, MH_KERNEL_CONVEXHULL,
  MH_KERNEL_THINSE, MH_KERNEL_SKELETON, MH_KERNEL_CHEBYSHEV, MH_KERNEL_MANHATTAN,
  MH_KERNEL_OCTAGONAL, MH_KERNEL_EUCLIDEAN, MH_KERNEL_USERDEFINED
} MhKernelInfoType;

/* Mirror of KernelInfo, MagickCore/morphology.h:100-127.  values is row-major
   height x width; NaN marks a cell that is not part of the neighbourhood. */
typedef struct MhKernelInfo
{
  MhKernelInfoType type;
  size_t width,height;
  ptrdiff_t x,y;
  double *values;
  double minimum,maximum,negative_range,positive_range,angle;
  struct MhKernelInfo *next;
} MhKernelInfo;

/* AcquireKernelInfo, morphology.c:485: "name:args" or "WxH+X+Y: v,v,..."
   kernel strings, ';'-separated lists.  NULL on parse failure / unsupported
   kernel name. */
MH_API MhKernelInfo *MhAcquireKernelInfo(const char *kernel_string);
MH_API MhKernelInfo *MhDestroyKernelInfo(MhKernelInfo *kernel);
MH_API MhKernelInfo *MhCloneKernelInfo(const MhKernelInfo *kernel);
/* ScaleKernelInfo, morphology.c:4571.  flags: 1 = Normalize, 2 = CorrelateNormalize */
MH_API void MhScaleKernelInfo(MhKernelInfo *kernel,double scaling_factor,unsigned flags);
/* GetOptimalKernelWidth1D / 2D, gem.c:262,302 */
MH_API size_t MhGetOptimalKernelWidth1D(double radius,double sigma);
MH_API size_t MhGetOptimalKernelWidth2D(double radius,double sigma);
/* The tables the edge-preserving blurs build on the host, for inspection.  Bilateral (effect.c:951-970):
   intensity_gaussian[511], entry d+255 for a difference d of two intensity bytes, and
   spatial_gaussian[W*H], W = max(width,1), H = max(height,1).  Selective (effect.c:3456-3466): returns
   GetOptimalKernelWidth1D(radius,sigma) and, unless kernel is NULL, fills kernel[width*width]. */
MH_API MhStatus MhBilateralBlurTables(size_t width,size_t height,double intensity_sigma,double spatial_sigma,
  double *intensity_gaussian,double *spatial_gaussian);
MH_API size_t MhSelectiveBlurKernel(double radius,double sigma,double *kernel);
/* Is the 2-D kernel an outer product column[y]*row[x] (to 1e-13 of its largest cell, no NaN
   cells)?  Returns 1 and fills row[width] / column[height] (either may be NULL), else 0.  FAST
   ConvolveImage runs such kernels (Gaussian:RxS, i.e. GaussianBlurImage) as two 1-D passes
   with one division at the end instead of morphology.c:2892-2979's width*height taps. */
MH_API int MhKernelOuterProductFactors(const MhKernelInfo *kernel,double *row,double *column);
/* ... or an outer product everywhere but at its origin cell (SharpenImage's negated Gaussian,
   EdgeImage's box of -1: effect.c:3640-3660, :1530-1545)?  Returns 1 (outer product, *delta = 0),
   2 (values[y][x] = column[y]*row[x] + *delta at the origin cell) or 0.  EXACT mode and float
   Quantum run both forms as two fp64 passes with a tie check, bit-identical to the w x h walk. */
MH_API int MhKernelOuterProductPlusDelta(const MhKernelInfo *kernel,double *row,double *column,
  double *delta);
/* Host test of the exact-integer 2-D convolve (MhConvolve2DRecomputed above): are the kernel's cells integer multiples (|m| <= 127) of one unit — every
   flat shape kernel after `convolve:scale`, binomial and hand-written integer kernels?  cells[]
   (width*height ints in the kernel's own order, NaN cells as 0; may be NULL) and *unit (may be NULL)
   receive the form values[i] = cells[i] * unit (to 1e-9 of a cell); returns 1 or 0. */
MH_API int MhKernelIntegerCells(const MhKernelInfo *kernel,int *cells,double *unit);

/* MorphologyMethod, MagickCore/morphology.h:72-98 (same values) */
typedef enum
{
  MH_MORPHOLOGY_UNDEFINED = 0,
  MH_MORPHOLOGY_CONVOLVE, MH_MORPHOLOGY_CORRELATE,
  MH_MORPHOLOGY_ERODE, MH_MORPHOLOGY_DILATE,
  MH_MORPHOLOGY_ERODE_INTENSITY, MH_MORPHOLOGY_DILATE_INTENSITY,
  MH_MORPHOLOGY_ITERATIVE_DISTANCE,
  MH_MORPHOLOGY_OPEN, MH_MORPHOLOGY_CLOSE,
  MH_MORPHOLOGY_OPEN_INTENSITY, MH_MORPHOLOGY_CLOSE_INTENSITY,
  MH_MORPHOLOGY_SMOOTH,
  MH_MORPHOLOGY_EDGE_IN, MH_MORPHOLOGY_EDGE_OUT, MH_MORPHOLOGY_EDGE,
  MH_MORPHOLOGY_TOP_HAT, MH_MORPHOLOGY_BOTTOM_HAT,
  MH_MORPHOLOGY_HIT_AND_MISS, MH_MORPHOLOGY_THINNING, MH_MORPHOLOGY_THICKEN,
  MH_MORPHOLOGY_DISTANCE, MH_MORPHOLOGY_VORONOI
} MhMorphologyMethod;

/* FilterType, MagickCore/resample.h:31-69 (same values) */
typedef enum
{
  MH_FILTER_UNDEFINED = 0,
  MH_FILTER_POINT, MH_FILTER_BOX, MH_FILTER_TRIANGLE, MH_FILTER_HERMITE,
  MH_FILTER_HANN, MH_FILTER_HAMMING, MH_FILTER_BLACKMAN, MH_FILTER_GAUSSIAN,
  MH_FILTER_QUADRATIC, MH_FILTER_CUBIC, MH_FILTER_CATROM, MH_FILTER_MITCHELL,
  MH_FILTER_JINC, MH_FILTER_SINC, MH_FILTER_SINCFAST, MH_FILTER_KAISER,
  MH_FILTER_WELCH, MH_FILTER_PARZEN, MH_FILTER_BOHMAN, MH_FILTER_BARTLETT,
  MH_FILTER_LAGRANGE, MH_FILTER_LANCZOS, MH_FILTER_LANCZOSSHARP,
  MH_FILTER_LANCZOS2, MH_FILTER_LANCZOS2SHARP, MH_FILTER_ROBIDOUX,
  MH_FILTER_ROBIDOUXSHARP, MH_FILTER_COSINE, MH_FILTER_SPLINE,
  MH_FILTER_LANCZOSRADIUS, MH_FILTER_CUBICSPLINE, MH_FILTER_MAGICKERNELSHARP2013,
  MH_FILTER_MAGICKERNELSHARP2021, MH_FILTER_SENTINEL
} MhFilterType;

/* ResizeFilter (opaque), resize.c:91-108; AcquireResizeFilter resize.c:803
   (cylindrical = False, no expert `filter:*` artifacts). */
typedef struct MhResizeFilter MhResizeFilter;
MH_API MhResizeFilter *MhAcquireResizeFilter(MhFilterType filter,int image_has_alpha_or_enlarging_hint);
/* A filter whose weights are evaluated by the caller: the MagickCore shim passes the
   reference's own GetResizeFilterWeight / GetResizeFilterSupport (resize.c:1690, :1668) for
   the ResizeFilter AccelerateResizeImage receives (accelerate-private.h:43-44), so expert
   `filter:*` artifacts are honoured.  The callback runs on the host while the tap tables are
   built (2*(columns+rows)*taps calls), never on the device. */
typedef double (*MhResizeWeightFunction)(void *user,double x);
MH_API MhResizeFilter *MhAcquireResizeFilterFromCallback(MhResizeWeightFunction weight,
  void *user,double support);
MH_API MhResizeFilter *MhDestroyResizeFilter(MhResizeFilter *filter);
MH_API double MhGetResizeFilterWeight(const MhResizeFilter *filter,double x);   /* resize.c:1690 */
MH_API double MhGetResizeFilterSupport(const MhResizeFilter *filter);           /* resize.c:1668 */

/* --------------------------------------------------------------- operators */
/*
  New-image operators take a caller-allocated destination whose geometry,
  quantum kind and channel layout the caller has set (CloneImage in the shim,
  accelerate.c:239-256); in-place operators mutate `image`.
*/

/* AccelerateBlurImage: BlurImage(image,radius,sigma), effect.c:765-796. */
MH_API MhStatus MagickHipBlurImage(const MhImage *image,MhImage *blur_image,
  double radius,double sigma);

/* ConvolveImage(image,kernel), effect.c:1170 -> MorphologyImage(Convolve,1). */
MH_API MhStatus MagickHipConvolveImage(const MhImage *image,MhImage *convolve_image,
  const MhKernelInfo *kernel);

/* The other callers of ConvolveImage: each builds its kernel on the host
   exactly as the reference does and runs MorphologyImage(Convolve,1).
     GaussianBlurImage  effect.c:1709-1735  kernel "gaussian:RxS"
     SharpenImage       effect.c:3991-4062  negated 2-D gaussian, centre -2*sum, normalised
     EdgeImage          effect.c:1523-1566  all -1, centre width*width-1 (width from sigma 0.5)
     EmbossImage        effect.c:1600-1678  anti-diagonal signed gaussian, then EqualizeImage */
MH_API MhStatus MagickHipGaussianBlurImage(const MhImage *image,MhImage *blur_image,
  double radius,double sigma);
MH_API MhStatus MagickHipSharpenImage(const MhImage *image,MhImage *sharp_image,
  double radius,double sigma);
MH_API MhStatus MagickHipEdgeImage(const MhImage *image,MhImage *edge_image,double radius);
MH_API MhStatus MagickHipEmbossImage(const MhImage *image,MhImage *emboss_image,
  double radius,double sigma);

/* AccelerateWaveletDenoiseImage: WaveletDenoiseImage(image,threshold,softness),
   visual-effects.c:3520-3760.  (The reference's hook drops `softness`; the shim's build-time
   patch passes it.)  Images below 33 pixels on a side are left to the CPU. */
MH_API MhStatus MagickHipWaveletDenoiseImage(const MhImage *image,MhImage *noise_image,
  double threshold,double softness);

/* AccelerateDespeckleImage: DespeckleImage(image), effect.c:1308-1490 (16 Hull sweeps). */
MH_API MhStatus MagickHipDespeckleImage(const MhImage *image,MhImage *despeckle_image);

/* StatisticType, statistic.h:139-152 (the same values) */
typedef enum
{
  MH_STATISTIC_UNDEFINED = 0,      /* StatisticImage's default branch: the mean */
  MH_STATISTIC_GRADIENT = 1,
  MH_STATISTIC_MAXIMUM = 2,
  MH_STATISTIC_MEAN = 3,
  MH_STATISTIC_MEDIAN = 4,
  MH_STATISTIC_MINIMUM = 5,
  MH_STATISTIC_MODE = 6,
  MH_STATISTIC_NONPEAK = 7,
  MH_STATISTIC_ROOT_MEAN_SQUARE = 8,
  MH_STATISTIC_STANDARD_DEVIATION = 9,
  MH_STATISTIC_CONTRAST = 10
} MhStatisticType;

/* AccelerateStatisticImage: StatisticImage(image,type,width,height), statistic.c:2918-3163;
   bit-identical in both precision modes, Q16 and float Quantum.  Output (x,y) is the statistic
   of the W x H window from (x-W/2, y-H/2), W = max(width,1), H = max(height,1), edge-clamped.
   Window limit: one channel of the workgroup's (W+15) x (H+15) window must fit 64 KiB of LDS at
   2 bytes a sample (median, mode, nonpeak; every type on Q16) or 4 bytes (the other types on
   float Quantum), i.e. up to 166 x 166 and 113 x 113 for square windows; W and H at most 4096.
   Larger windows return MH_UNSUPPORTED (the CPU path runs). */
MH_API MhStatus MagickHipStatisticImage(const MhImage *image,MhImage *statistic_image,
  MhStatisticType type,size_t width,size_t height);

/* BilateralBlurImage(image,width,height,intensity_sigma,spatial_sigma), effect.c:894-1142 (the
   reference has no accelerate hook for it); bit-identical in both precision modes, Q16 and float
   Quantum.  W = max(width,1) and H = max(height,1) must be odd: with an even side the reference's
   reflected walk reads a column and a row outside the window it fetched, and the call returns
   MH_UNSUPPORTED (the CPU path runs).  One table entry is restated differently on purpose:
   intensity_gaussian[510], the weight of a tap whose intensity byte is 255 above the centre's, is
   never written by the reference (an uninitialised stack slot); here it is
   BlurGaussian(255,intensity_sigma).  Window limit: the workgroup's (W+15) x (H+15) tile, at
   channels*sizeof(Quantum)+1 bytes a pixel behind a 4 KiB table, must fit 128 KiB of LDS: up to
   69 x 69 for RGBA float Quantum, 101 x 101 for RGBA Q16; larger windows return MH_UNSUPPORTED.
   NaN samples are out of scope. */
MH_API MhStatus MagickHipBilateralBlurImage(const MhImage *image,MhImage *blur_image,
  size_t width,size_t height,double intensity_sigma,double spatial_sigma);

/* SelectiveBlurImage(image,radius,sigma,threshold), effect.c:3406-3710 (no accelerate hook in the
   reference either); bit-identical in both precision modes, Q16 and float Quantum.  threshold is
   in Quantum units (the CLI's percent conversion is the caller's).  Served: gray images and
   three-colour images in sRGB or linear RGB, with or without alpha; other colourspaces return
   MH_UNSUPPORTED.  Window limit: the (width+15)^2 tile at channels*sizeof(Quantum)+8 bytes a pixel
   (+16 with blending alpha) must fit 128 KiB of LDS: up to 49 x 49 for RGBA float Quantum, 57 x 57
   for RGBA Q16; larger kernels return MH_UNSUPPORTED.  NaN samples are out of scope. */
MH_API MhStatus MagickHipSelectiveBlurImage(const MhImage *image,MhImage *blur_image,
  double radius,double sigma,double threshold);

/* KuwaharaImage(image,radius,sigma), effect.c:1775-1978 (no accelerate hook in the reference);
   bit-identical in both precision modes, Q16 and float Quantum, 1-4 channels.  The operator's own
   BlurImage(image,radius,sigma) always runs as the bit-identical one, whatever MhImage::precision or
   MhSetPrecision say: the selection behind it is discrete (the quadrant of least luma variance,
   strict <), so a blur that is one level off can move the result by any amount.  What
   MagickHipBlurImage declines for (radius,sigma), this call declines too.  Restated: the default
   interpolation (the bilinear branch of InterpolatePixelChannels, every channel, alpha-weighted where
   the channel's trait carries Blend) and edge virtual pixels.  Window limit, w = (size_t) radius+1:
   the workgroup's (14+2w)^2 tile (15+2w for w <= 2) at channels*sizeof(Quantum)+8 bytes a pixel plus
   8*(15+w)^2 bytes of variances must fit 128 KiB of LDS: radius < 27 for RGBA float Quantum,
   radius < 34 for RGBA Q16; larger radii (and negative ones) return MH_UNSUPPORTED with the
   destination untouched.  NaN and infinite samples are out of scope. */
MH_API MhStatus MagickHipKuwaharaImage(const MhImage *image,MhImage *kuwahara_image,
  double radius,double sigma);

/* AccelerateLocalContrastImage: LocalContrastImage(image,radius,strength), effect.c:1760-2010.
   MH_UNSUPPORTED (CPU path) when the blur width 0.002*max(columns,rows)*|radius| is 0 or does
   not leave room for the mirrored padding. */
MH_API MhStatus MagickHipLocalContrastImage(const MhImage *image,MhImage *contrast_image,
  double radius,double strength);

/* AccelerateRotationalBlurImage: RotationalBlurImage(image,angle), effect.c:3209-3430. */
MH_API MhStatus MagickHipRotationalBlurImage(const MhImage *image,MhImage *blur_image,double angle);

/* AccelerateMotionBlurImage: MotionBlurImage, effect.c:2347-2560.  The first form builds the
   kernel (GetMotionBlurKernel, :2316-2345) and the offsets along `angle` (:2385-2393) itself;
   the second takes them from the caller, as the reference's accelerate hook does
   (`offsets_xy` = width pairs x,y). */
MH_API MhStatus MagickHipMotionBlurImage(const MhImage *image,MhImage *blur_image,double radius,
  double sigma,double angle);
MH_API MhStatus MagickHipMotionBlurImageWithKernel(const MhImage *image,MhImage *blur_image,
  const double *kernel,size_t width,const ptrdiff_t *offsets_xy);

/* MorphologyImage / MorphologyApply, morphology.c:4129 / :3634, with the per-method default
   handling of multi-kernel results (re-iterate; HitAndMiss: Lighten union); `bias` is the
   convolve:bias artifact (0 by default). */
MH_API MhStatus MagickHipMorphologyImage(const MhImage *image,MhImage *morphology_image,
  MhMorphologyMethod method,ptrdiff_t iterations,const MhKernelInfo *kernel,
  double bias);

/* The same with the user's `morphology:compose` (morphology.c:4206-4215, :3779-3782): how the
   results of the kernels of a list are merged.  DEFAULT = UndefinedCompositeOp, NONE =
   NoCompositeOp (re-iterate the previous result), LIGHTEN / DIFFERENCE / DARKEN / PLUS / MULTIPLY /
   SCREEN / EXCLUSION / MINUS_SRC / MINUS_DST / LINEAR_DODGE / OVER / DST_OVER = CompositeImage with
   that operator (composite.c:2396-3124, synchronised channels).
   Other operators: MH_UNSUPPORTED (the CPU path runs). */
typedef enum
{
  MH_MORPHOLOGY_COMPOSE_DEFAULT = 0,
  MH_MORPHOLOGY_COMPOSE_NONE = 1,
  MH_MORPHOLOGY_COMPOSE_LIGHTEN = 2,
  MH_MORPHOLOGY_COMPOSE_DIFFERENCE = 3,
  MH_MORPHOLOGY_COMPOSE_OTHER = 4,
  MH_MORPHOLOGY_COMPOSE_DARKEN = 5,
  MH_MORPHOLOGY_COMPOSE_PLUS = 6,      /* `-define morphology:compose=Plus`, morphology.c:772 */
  MH_MORPHOLOGY_COMPOSE_MULTIPLY = 7,
  MH_MORPHOLOGY_COMPOSE_SCREEN = 8,
  MH_MORPHOLOGY_COMPOSE_EXCLUSION = 9,
  MH_MORPHOLOGY_COMPOSE_MINUS_SRC = 10,
  MH_MORPHOLOGY_COMPOSE_MINUS_DST = 11,
  MH_MORPHOLOGY_COMPOSE_LINEAR_DODGE = 12,
  MH_MORPHOLOGY_COMPOSE_OVER = 13,     /* OverCompositeOp and SrcOverCompositeOp: CompositeOverImage, composite.c:917 */
  MH_MORPHOLOGY_COMPOSE_DST_OVER = 14
} MhMorphologyCompose;
MH_API MhStatus MagickHipMorphologyImageCompose(const MhImage *image,MhImage *morphology_image,
  MhMorphologyMethod method,ptrdiff_t iterations,const MhKernelInfo *kernel,
  double bias,MhMorphologyCompose compose);

/* One MorphologyPrimitive pass (morphology.c:2566) with a single kernel;
   *changed receives the reference's return value. */
MH_API MhStatus MagickHipMorphologyPrimitive(const MhImage *image,MhImage *morphology_image,
  MhMorphologyMethod method,const MhKernelInfo *kernel,double bias,
  ptrdiff_t *changed);

/* AccelerateUnsharpMaskImage: UnsharpMaskImage, effect.c:4256-4400. */
MH_API MhStatus MagickHipUnsharpMaskImage(const MhImage *image,MhImage *unsharp_image,
  double radius,double sigma,double gain,double threshold);

/* AccelerateResizeImage: ResizeImage, resize.c:3761-3874.  resize_image
   carries the target columns/rows. */
MH_API MhStatus MagickHipResizeImage(const MhImage *image,MhImage *resize_image,
  MhFilterType filter);
/* As above with a filter object (what the shim passes after AcquireResizeFilter). */
MH_API MhStatus MagickHipResizeImageWithFilter(const MhImage *image,MhImage *resize_image,
  const MhResizeFilter *filter);

/* SampleImage, resize.c:3907-4075: sample_image carries the target columns/rows.  Every defined channel
   is copied verbatim from column (ssize_t) (((x+offset)*columns)/sample_columns), rows alike, with
   offset = percent/100-MagickEpsilon (the sample:offset artifact); a negative percentage means the
   default, 0.5-MagickEpsilon.  Percentages above 100, and any geometry whose offsets leave the frame,
   would read virtual pixels: MH_UNSUPPORTED, destination untouched.  A same-size request copies.
   Bit-identical in both precision modes. */
MH_API MhStatus MagickHipSampleImage(const MhImage *image,MhImage *sample_image,double offset_x_percent,
  double offset_y_percent);
/* ScaleImage, resize.c:4106-4536: the reference's two serial state machines depend on the four
   dimensions only, so every output sample is a short ordered fp64 sum whose terms a host plan lists
   (MhScaleImagePlan); the device evaluates them in the reference's order.  Bit-identical in both
   precision modes, Q16 and float Quantum.  A same-size request copies.  MH_UNSUPPORTED (destination
   untouched) for a geometry in which the reference leaves a destination column unset or stores past its
   scanline; none is known. */
MH_API MhStatus MagickHipScaleImage(const MhImage *image,MhImage *scale_image);
/* ThumbnailImage's pixel work, resize.c:4627-4649: with the integer factors columns/thumbnail columns
   and rows/thumbnail rows both above 4 SampleImage to four times the target, both above 2
   ResizeImage(Box) to twice the target, then ResizeImage(filter) to the target (MH_FILTER_UNDEFINED:
   LanczosSharp).  The intermediates stay on the device.  When both resizes run, the Box stage runs in
   MH_PRECISION_EXACT whatever the mode, so the result keeps ResizeImage's contract. */
MH_API MhStatus MagickHipThumbnailImage(const MhImage *image,MhImage *thumbnail_image,MhFilterType filter);
/* ScaleImage's plan for one axis (host only, no device needed).  axis 0: rows (the y_vector / span.y
   machine), axis 1: columns (the scale_scanline machine).  counts[d] receives the number of terms of
   destination sample d; indices / weights receive the terms of sample 0, then sample 1, ... in the order
   the reference adds them, each sum starting from 0.0; at most `capacity` terms are written.  An axis
   with source == destination has no terms: the reference does no arithmetic there.  Returns the total
   number of terms, -1 for a zero dimension, -2 when the plan is not realisable (see MagickHipScaleImage). */
MH_API long long MhScaleImagePlan(size_t source,size_t destination,int axis,unsigned *counts,int *indices,
  double *weights,size_t capacity);
/* SampleImage's offset table for one axis (host only); returns 0, or -1 when an offset leaves
   [0, source) or the percentage is above 100 (negative: the default). */
MH_API int MhSampleImageOffsets(size_t source,size_t destination,double offset_percent,long long *offsets);

/* AccelerateContrastStretchImage: ContrastStretchImage, enhance.c:1544-1818.
   black_point / white_point are pixel counts as in the MagickCore API.
   *became_gray (optional) reports the IdentifyImageType side effect
   (enhance.c:1586-1588): when set, the caller must SetImageColorspace(GRAY). */
MH_API MhStatus MagickHipContrastStretchImage(MhImage *image,double black_point,
  double white_point,int *became_gray);

/* AccelerateEqualizeImage: EqualizeImage, enhance.c:2040-2280. */
MH_API MhStatus MagickHipEqualizeImage(MhImage *image);

/* CLAHEImage(image,width,height,number_bins,clip_limit), enhance.c:295-785 (no accelerate hook in
   the reference), in place: TransformImageColorspace to Lab, contrast-limited adaptive histogram
   equalisation of L over width x height tiles (0: columns>>3 / rows>>3; the frame padded to whole
   tiles by edge replication; number_bins 0: 128, at most 256), TransformImageColorspace back;
   image->colorspace ends at its value on entry.  An image already in Lab runs the core alone.
   Host or device memory, Q16 and float Quantum, R,G,B[,A] layouts in every colourspace
   MagickHipTransformImageColorspace converts to and from Lab.  Both conversions always run as the
   bit-identical ones, whatever MhImage::precision or MhSetPrecision say: one level of L across a
   bin boundary moves a histogram count and the mapped value by a whole bin step.  The channel mask
   and the traits play no part, as in the reference.
   Q16: bit-identical to the reference.  Float Quantum: the core is bit-identical on any frame
   (so a Lab image is); from another colourspace the call equals, bit for bit, this library's own
   MagickHipTransformImageColorspace(Lab) -> the core -> MagickHipTransformImageColorspace(back),
   and those float conversions are within 1 ULP of the reference's libm (the library's contract for
   them), so the whole is not promised bit-identical to the CPU there.
   MH_UNSUPPORTED (image untouched; the CPU path runs): one- and two-channel frames and four plain
   channels, a colourspace that is not accelerated, tile maps (tiles x bins x 2 bytes) larger than
   the frame, a padded frame of 2^32 pixels or more, a negative or NaN clip_limit.
   MH_BAD_ARGUMENT (the reference divides by zero): a resolved tile width or height of 0
   (columns < 8 with width 0), number_bins 1. */
MH_API MhStatus MagickHipCLAHEImage(MhImage *image,size_t width,size_t height,size_t number_bins,
  double clip_limit);

/* ---- The threshold operators, MagickCore/threshold.c (no accelerate hook in the reference).
   Every result is a comparison, so all of them are bit-identical to the reference in both
   precision modes, on Q16 and float Quantum, 1-4 channels, host and device memory.  NaN and
   infinite samples are outside the contract.
   The pointwise calls form `pixel` = GetPixelIntensity (MhImage::intensity, colorspace) once per
   pixel; with a channel_mask other than MH_ALL_CHANNELS every channel is decided by its own sample
   instead.  Only channels whose trait carries MH_TRAIT_UPDATE are written. */

/* AutoThresholdMethod, MagickCore/threshold.h:25-31 */
typedef enum
{
  MH_AUTO_THRESHOLD_UNDEFINED = 0,
  MH_AUTO_THRESHOLD_KAPUR = 1,
  MH_AUTO_THRESHOLD_OTSU = 2,
  MH_AUTO_THRESHOLD_TRIANGLE = 3
} MhAutoThresholdMethod;

/* BilevelImage(image,threshold), threshold.c:805-896, in place: pixel <= threshold ? 0 : QuantumRange.
   A frame outside the gray colourspaces is retagged sRGB first, as SetImageColorspace does there:
   image->colorspace ends at MH_COLORSPACE_SRGB. */
MH_API MhStatus MagickHipBilevelImage(MhImage *image,double threshold);

/* AutoThresholdImage(image,method), threshold.c:660-762, in place: 256 counts of
   ScaleQuantumToChar(ClampToQuantum(intensity)) gathered on the device, the selection
   (MhAutoThresholdFromHistogram) on the host, then BilevelImage at QuantumRange*percent/100.
   *threshold_percent (optional) receives the value the reference formats into the
   "auto-threshold:threshold" property.  A method outside the three takes OTSU, as the reference's
   `default:` does. */
MH_API MhStatus MagickHipAutoThresholdImage(MhImage *image,MhAutoThresholdMethod method,
  double *threshold_percent);

/* The host half of AutoThresholdImage, threshold.c:392-658 and :718-748: normalisation by
   PerceptibleReciprocal(sum) and the Kapur / OTSU / Triangle selection, operation for operation
   (log, pow and sqrt of the host's libm).  counts: the 256 bins.  No device is touched. */
MH_API MhStatus MhAutoThresholdFromHistogram(const double counts[256],MhAutoThresholdMethod method,
  double *threshold_percent);

/* AdaptiveThresholdImage(image,width,height,bias), threshold.c:182-361: threshold_image(x,y) =
   centre <= sum/(width*height)+bias ? 0 : QuantumRange over the window of columns x-width/2 ...
   x-width/2+width-1 and rows y-height/2 ... y-height/2+height-1, edge-clamped.  Channels whose
   trait in threshold_image carries MH_TRAIT_COPY (or is undefined on either side) receive the
   source sample.  width == 0 or height == 0: a copy of the source.
   Q16: exact integer window sums.  Float Quantum: the reference's running sum, statement for
   statement, one sequential chain per row and channel (slower).
   MH_UNSUPPORTED (threshold_image untouched; the CPU path runs): Q16 with width > 257 (a strip of
   512 input columns keeps at least 256 outputs: width <= 512/2+1) or height > 65537 (a column sum
   of height samples fits 32 bits: height*65535 < 2^32); float Quantum with a side above 2^20; a
   frame side above 2^30-1. */
MH_API MhStatus MagickHipAdaptiveThresholdImage(const MhImage *image,MhImage *threshold_image,size_t width,
  size_t height,double bias);

/* BlackThresholdImage :927-1058 (pixel < threshold: 0) and WhiteThresholdImage :2518-2648
   (pixel > threshold: QuantumRange), in place.  thresholds[c]: the threshold of the channel stored
   at offset c, in Quantum units; the geometry string and its percent flag stay with the caller.
   MH_UNSUPPORTED (image untouched): a frame in a gray colourspace or with fewer than three colour
   channels, which the reference re-lays out as sRGB first. */
MH_API MhStatus MagickHipBlackThresholdImage(MhImage *image,const double thresholds[MH_MAX_CHANNELS]);
MH_API MhStatus MagickHipWhiteThresholdImage(MhImage *image,const double thresholds[MH_MAX_CHANNELS]);

/* RangeThresholdImage(image,low_black,low_white,high_white,high_black), threshold.c:2377-2487, in
   place, branch for branch; the ramps are ClampToQuantum(QuantumRange*PerceptibleReciprocal(d)*
   (pixel-low)) in that order in fp64.  MH_UNSUPPORTED: gray frames, as above. */
MH_API MhStatus MagickHipRangeThresholdImage(MhImage *image,double low_black,double low_white,
  double high_white,double high_black);

/* TransformImageColorspace, colorspace.c:1751 — sRGB <-> linear RGB / Lab / XYZ.
   On success image->colorspace is updated. */
MH_API MhStatus MagickHipTransformImageColorspace(MhImage *image,MhColorspace colorspace);

/* AccelerateGrayscaleImage (accelerate-private.h:58-59): GrayscaleImage, enhance.c:2476-2660.
   Writes the intensity to the first channel; the caller then sets the image's colourspace to
   GRAY (LinearGRAY for the two Luminance methods) as enhance.c:2502-2510 does. */
MH_API MhStatus MagickHipGrayscaleImage(MhImage *image,MhIntensityMethod method);

/* MagickFunction, MagickCore/statistic.h:129-136 (same values) */
typedef enum
{
  MH_FUNCTION_UNDEFINED = 0,
  MH_FUNCTION_ARCSIN,
  MH_FUNCTION_ARCTAN,
  MH_FUNCTION_POLYNOMIAL,
  MH_FUNCTION_SINUSOID
} MhFunction;

/* StorageType, MagickCore/pixel.h:146-156 (same values) */
typedef enum
{
  MH_STORAGE_UNDEFINED = 0,
  MH_STORAGE_CHAR, MH_STORAGE_DOUBLE, MH_STORAGE_FLOAT, MH_STORAGE_LONG, MH_STORAGE_LONGLONG,
  MH_STORAGE_QUANTUM, MH_STORAGE_SHORT
} MhStorageType;

/* ImportImagePixels / ExportImagePixels, pixel.c:4164 / :1962: converts between
   the caller's interleaved component buffer and the Quantum pixels of `image`, for the region
   x,y,width,height (inside the image).  `map` lists the buffer's components, any order of
   R,G,B,A,O (= alpha),I (gray / intensity),P (pad); C,M,Y,K are not accelerated.  `pixels` is
   width*height*strlen(map) tightly packed elements of `type`, in host or device memory
   (`pixels_memory`).  The image must already have the layout the map implies (alpha channel
   present for A/O; the reference's side effects on alpha_trait / colourspace are the caller's). */
MH_API MhStatus MagickHipImportImagePixels(MhImage *image,ptrdiff_t x,ptrdiff_t y,size_t width,
  size_t height,const char *map,MhStorageType type,const void *pixels,MhMemoryKind pixels_memory);
MH_API MhStatus MagickHipExportImagePixels(const MhImage *image,ptrdiff_t x,ptrdiff_t y,
  size_t width,size_t height,const char *map,MhStorageType type,void *pixels,
  MhMemoryKind pixels_memory);

/* AccelerateContrastImage: ContrastImage(image,sharpen), enhance.c:1392-1480 — brightness
   pushed along a sine in HSB (Contrast(), :1370-1390).  R,G,B[,A] layouts. */
MH_API MhStatus MagickHipContrastImage(MhImage *image,int sharpen);

/* AccelerateModulateImage: ModulateImage's pixel loop, enhance.c:3776-3860, for the HSL
   (default, colorspace = MH_COLORSPACE_UNDEFINED or MH_COLORSPACE_HSL) and HSB models.  The
   three percentages are the parsed "brightness,saturation,hue" geometry (100 = unchanged). */
MH_API MhStatus MagickHipModulateImage(MhImage *image,double percent_brightness,
  double percent_saturation,double percent_hue,int colorspace);

/* AccelerateFunctionImage (accelerate-private.h:56-57): FunctionImage / ApplyFunction,
   statistic.c:975-1160, on every channel whose trait carries Update. */
MH_API MhStatus MagickHipFunctionImage(MhImage *image,MhFunction function,
  size_t number_parameters,const double *parameters);

/* ---- The level operators, MagickCore/enhance.c and histogram.c (no accelerate hook in the
   reference).  All in place, 1-4 channels, host and device memory, both Quantum
   types.  Only channels whose trait carries MH_TRAIT_UPDATE are written.  fp64 in the
   reference's operation order.  Q16 results are bit-identical to the reference in both precision
   modes: a curve that calls libm (gamma != 1, the sigmoidals) is tabulated over the 65536 samples
   on the host, with the host's libm, and applied as a table; a few tables are kept per process.
   Float Quantum is evaluated on the device: bit-identical where no libm is involved (gamma == 1,
   NegateImage) and for GammaImage (table-driven in the reference too), within one float ULP where
   the device's pow / tanh / atanh is.  There is no FAST variant.  NaN and infinite samples are
   outside the contract. */

/* LevelImage(image,black_point,white_point,gamma), enhance.c:2913-3018:
   ClampToQuantum(QuantumRange*gamma_pow(PerceptibleReciprocal(white-black)*(q-black),
   PerceptibleReciprocal(gamma))), gamma_pow(v,g) = v < 0 ? v : pow(v,g); then ClampImage: a float
   result below 0 becomes 0, one at or above QuantumRange becomes QuantumRange. */
MH_API MhStatus MagickHipLevelImage(MhImage *image,double black_point,double white_point,double gamma);

/* LevelizeImage, enhance.c:3062-3170: ClampToQuantum(gamma_pow(QuantumScale*q,gamma)*(white-black)+
   black); no ClampImage: float results may leave the range. */
MH_API MhStatus MagickHipLevelizeImage(MhImage *image,double black_point,double white_point,double gamma);

/* GammaImage, enhance.c:2322-2440: gamma == 1 leaves the frame untouched; otherwise
   map[ScaleQuantumToMap(ClampToQuantum(q))] with the map of MhGammaLUT, on both Quantum types.
   image->gamma *= gamma is the caller's side effect. */
MH_API MhStatus MagickHipGammaImage(MhImage *image,double gamma);

/* NegateImage(image,grayscale), enhance.c:3940-4100: QuantumRange-q; with grayscale != 0 only in
   pixels whose |R-G| and |G-B| are below MagickEpsilon (IsPixelGray: every pixel of a frame with
   fewer than three colour channels). */
MH_API MhStatus MagickHipNegateImage(MhImage *image,int grayscale);

/* SigmoidalContrastImage(image,sharpen,contrast,midpoint), enhance.c:4267-4407, the tanh / atanh
   form; midpoint in Quantum units.  contrast < MagickEpsilon leaves the frame untouched. */
MH_API MhStatus MagickHipSigmoidalContrastImage(MhImage *image,int sharpen,double contrast,double midpoint);

/* GetImageRange, statistic.c:1851-1929, with its seed: every row starts from the offset-0 sample
   of its first pixel whatever the mask, so the range is over the samples of the Update channels
   AND column 0 of channel 0; *maximum starts at MagickMinimumValue (2.2e-308), *minimum at
   MagickMaximumValue. */
MH_API MhStatus MagickHipImageRange(const MhImage *image,double *minimum,double *maximum);

/* MinMaxStretchImage(image,black,white,gamma), histogram.c:927-975.  channel_mask ==
   MH_ALL_CHANNELS: one range over the Update channels, min += black, max -= white, LevelImage
   unless |min-max| < MagickEpsilon.  Any other mask: for every offset whose trait carries Update,
   in order, the range and the LevelImage of that channel alone; the reference selects it with the
   ChannelType bit 1 << offset, which names no stored channel at the alpha offset: alpha is never
   levelled in this mode.  Channel 0 is levelled before the later channels are measured, and its
   column 0 is part of their range.  AutoLevelImage (enhance.c:187) is (0,0,1). */
MH_API MhStatus MagickHipMinMaxStretchImage(MhImage *image,double black,double white,double gamma);
MH_API MhStatus MagickHipAutoLevelImage(MhImage *image);

/* LinearStretchImage(image,black_point,white_point), enhance.c:3347-3427; the points are pixel
   counts.  65536 counts of ScaleQuantumToMap(ClampToQuantum(intensity)) on the device, the scan on
   the host, then LevelImage(ScaleMapToQuantum(black),ScaleMapToQuantum(white),1).  *black and
   *white (optional) receive the two bins: the reference's "histogram:linear-stretch" property is
   "%gx%g%%" of 100.0*black/MaxMap and 100.0*white/MaxMap. */
MH_API MhStatus MagickHipLinearStretchImage(MhImage *image,double black_point,double white_point,
  size_t *black,size_t *white);

/* NormalizeImage, enhance.c:4130-4140: ContrastStretchImage at 0.02 and 0.99 of the pixel count
   (MagickHipContrastStretchImage: MH_UNSUPPORTED for a colour frame whose pixels are all gray). */
MH_API MhStatus MagickHipNormalizeImage(MhImage *image);

/* BrightnessContrastImage, enhance.c:224-252: FunctionImage(Polynomial) with slope and intercept. */
MH_API MhStatus MagickHipBrightnessContrastImage(MhImage *image,double brightness,double contrast);

/* Tone-curve tables built by this process so far (a call whose parameters hit the cache builds none). */
MH_API unsigned long long MhLevelsTablesBuilt(void);

/* ---------------------------------------------------------- building blocks */
/* Exposed so a row-sharded image (one band per GPU / per process) can run the
   global-histogram operators with one all-reduce between the phases
   (SURVEY §8e): histogram -> [all-reduce] -> LUT -> apply. */

#define MH_MAXMAP 65535u
#define MH_HISTOGRAM_BINS (MH_MAXMAP+1u)

/* histogram[bin*number_channels + c], uint64 counts.
   mode 0: each channel bins its own value; mode 1: every channel bins the
   pixel intensity (enhance.c:1637-1643, :2125-2129).  Accumulates into
   `histogram` (caller zeroes it).  histogram follows image->memory. */
MH_API MhStatus MagickHipHistogram(const MhImage *image,int intensity_mode,uint64_t *histogram);

/* Host-side LUT builders (pure C, no device).  lut[bin*number_channels + c],
   in Quantum units as double; apply_mask bit c is cleared when channel c must
   be left untouched (black == white). */
MH_API MhStatus MhContrastStretchLUT(const uint64_t *histogram,uint32_t number_channels,
  size_t columns,size_t rows,double black_point,double white_point,
  MhQuantumKind quantum,double *lut,uint32_t *apply_mask);
MH_API MhStatus MhEqualizeLUT(const uint64_t *histogram,uint32_t number_channels,
  MhQuantumKind quantum,double *lut,uint32_t *apply_mask);

/* GammaImage's map, enhance.c:2354-2362: lut[i] = ScaleMapToQuantum(MaxMap*pow(i/MaxMap,
   PerceptibleReciprocal(gamma))) for the 65536 bins, all zero when gamma == 0; one column. */
MH_API MhStatus MhGammaLUT(double gamma,MhQuantumKind quantum,double *lut);

/* q[c] = ClampToQuantum(lut[ScaleQuantumToMap(q[c])*number_channels + c]) for
   Update channels selected by apply_mask (enhance.c:1778-1788, :2252-2262).
   `lut` is a host pointer. */
MH_API MhStatus MagickHipApplyLUT(MhImage *image,const double *lut,uint32_t apply_mask);

/* The second half of EqualizeImage (equalize != 0) / ContrastStretchImage for a caller that
   already holds the histogram — e.g. the table all-reduced over the row bands of a sharded
   image: LUT construction (enhance.c:1652-1706, :2138-2169) and application on the
   device.  `histogram` follows image->memory; image_rows = rows of the WHOLE image (0: this
   image's), whose pixel count the white point refers to. */
MH_API MhStatus MagickHipApplyHistogram(MhImage *image,const uint64_t *histogram,int intensity_mode,
  int equalize,double black_point,double white_point,size_t image_rows);

/* TransformImageColorspace(image, colorspace) followed by ContrastStretchImage(image, black_point,
   white_point) — colorspace.c:1751-1783 then enhance.c:1544-1818 — as one call with the two
   calls' results.  What the pair can share is the pass over the pixels: a FAST sRGB -> Lab of a
   device-resident RGBA Q16 frame converts and bins the intensity of what it stores in one kernel
   (BASELINE configs[3]: one frame read + one frame write before the map is applied).  Any other
   combination runs the two operators one after the other.  MagickHipBatchImages uses it for
   adjacent MH_OP_COLORSPACE / MH_OP_CONTRAST_STRETCH operators. */
MH_API MhStatus MagickHipTransformColorspaceContrastStretchImage(MhImage *image,MhColorspace colorspace,
  double black_point,double white_point);

/* IdentifyImageGray scan (attribute.c:1564-1626): *is_gray = 1 when every
   pixel has |R-G| and |G-B| below MagickEpsilon. */
MH_API MhStatus MagickHipIsImageGray(const MhImage *image,int *is_gray);

/* ------------------------------------------------- batches and several GPUs */
/*
  SURVEY section 8e.  The reference arbitrates devices and in-order queues per call
  (RequestOpenCLDevice, MagickCore/opencl.c:3056-3102; AcquireOpenCLCommandQueue, :656; 16
  queues per device, opencl-private.h:70) but hands every operator exactly one device.  These
  two entry points take a CHAIN of operators and spread the work over the GPUs of the node
  from plain C:

    MagickHipBatchImages    independent images (BASELINE config C4): a work queue over
                            devices x streams_per_device host threads, each with its own
                            stream, so the upload of one image, the kernels of another and the
                            download of a third overlap on every device.  No collective.
    MagickHipShardedImage   ONE large image cut into row bands, one per device (config C5):
                            stencil operators exchange their halo rows between neighbouring
                            bands with hipMemcpyPeerAsync before each pass; ContrastStretch and
                            Equalize bin their band, all-reduce the 65536 x channels table
                            (RCCL ncclAllReduce when the bands sit on different GPUs and
                            librccl loads, peer copies + an add kernel otherwise) and build and
                            apply the identical LUT on every device.

  number_devices <= 0 means MhDeviceCount().  More logical devices than physical ones are
  mapped round-robin (logical d runs on physical d mod MhDeviceCount()): that is how the test
  suite rehearses both entry points on a single GPU.

  What the two entry points do with each operator kind is one row of a table in batch.cpp (DESIGN.md
  section 5): whether the kind works in place, makes a new image of the same geometry or one of
  args[0] x args[1] (resize, sample, scale, thumbnail: the chain needs result descriptors), how many
  rows a stencil reaches, and whether MagickHipShardedImage runs it or returns MH_UNSUPPORTED, with
  the reason in MhGetLastError().
*/
typedef enum
{
  MH_OP_BLUR = 1,              /* args: radius, sigma */
  MH_OP_GAUSSIAN_BLUR = 2,     /* args: radius, sigma */
  MH_OP_UNSHARP_MASK = 3,      /* args: radius, sigma, gain, threshold */
  MH_OP_RESIZE = 4,            /* args: columns, rows, MhFilterType */
  MH_OP_MORPHOLOGY = 5,        /* args: MhMorphologyMethod, iterations, bias; text: kernel string */
  MH_OP_COLORSPACE = 6,        /* args: MhColorspace */
  MH_OP_CONTRAST_STRETCH = 7,  /* args: black_point, white_point (pixel counts, enhance.c:1544) */
  MH_OP_EQUALIZE = 8,
  MH_OP_STATISTIC = 9,         /* args: MhStatisticType, width, height */
  MH_OP_BILATERAL_BLUR = 10,   /* args: width, height, intensity_sigma, spatial_sigma */
  MH_OP_SELECTIVE_BLUR = 11,   /* args: radius, sigma, threshold */
  MH_OP_KUWAHARA = 12,         /* args: radius, sigma */
  MH_OP_CLAHE = 13,            /* args: width, height, number_bins, clip_limit */
  MH_OP_THRESHOLD = 14,        /* args: threshold (BilevelImage) */
  MH_OP_AUTO_THRESHOLD = 15,   /* args: MhAutoThresholdMethod */
  MH_OP_ADAPTIVE_THRESHOLD = 16, /* args: width, height, bias */
  MH_OP_LEVEL = 17,            /* args: black_point, white_point, gamma */
  MH_OP_LEVELIZE = 18,         /* args: black_point, white_point, gamma */
  MH_OP_GAMMA = 19,            /* args: gamma */
  MH_OP_NEGATE = 20,           /* args: grayscale */
  MH_OP_SIGMOIDAL_CONTRAST = 21, /* args: sharpen, contrast, midpoint */
  MH_OP_AUTO_LEVEL = 22,
  MH_OP_LINEAR_STRETCH = 23,   /* args: black_point, white_point (pixel counts) */
  MH_OP_NORMALIZE = 24,
  MH_OP_SAMPLE = 25,           /* args: columns, rows (default sample:offset) */
  MH_OP_SCALE = 26,            /* args: columns, rows */
  MH_OP_THUMBNAIL = 27         /* args: columns, rows, MhFilterType */
} MhOperatorKind;

typedef struct MhOperator
{
  uint32_t kind;               /* MhOperatorKind */
  double args[4];
  const char *text;
} MhOperator;

typedef struct MhBatchReport
{
  uint32_t devices;            /* logical devices used */
  uint32_t workers;            /* host threads = devices x streams per device */
  uint32_t used_rccl;          /* MagickHipShardedImage: the table went through ncclAllReduce */
  uint32_t halo_exchanges;     /* MagickHipShardedImage: hipMemcpyPeerAsync halo copies issued */
  uint64_t images_per_device[16];
  double seconds;              /* wall time of the call */
} MhBatchReport;

/* results[i] = operators(images[i]).  images / results: host or device memory; results[i]
   carries the geometry of the chain's output (equal to the input's unless the chain resizes).
   results == NULL: the chain must keep the geometry and images[i] is overwritten.
   Returns the first non-OK status of any image (the others still run). */
MH_API MhStatus MagickHipBatchImages(const MhOperator *operators,size_t number_operators,
  const MhImage *images,MhImage *results,size_t number_images,int number_devices,
  int streams_per_device,MhBatchReport *report);

/* result = operators(image) with the rows of `image` sharded over number_devices bands.
   Geometry-preserving operators only (no MH_OP_RESIZE); host or device memory. */
MH_API MhStatus MagickHipShardedImage(const MhOperator *operators,size_t number_operators,
  const MhImage *image,MhImage *result,int number_devices,MhBatchReport *report);

#if defined(__cplusplus)
}
#endif

#endif /* MAGICKHIP_H */
