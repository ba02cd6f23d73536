/*
  accelerate_hip.c — the MagickCore side of the MI355X accelerate backend.

  This file REPLACES MagickCore/accelerate.c in a MagickCore build whose
  OpenCL call sites are switched on (-DMAGICKCORE_HAVE_CL_CL_H=1 =>
  MAGICKCORE_OPENCL_SUPPORT, MagickCore/studio.h:149-154).  It defines the
  fourteen Accelerate*Image() entry points MagickCore/accelerate-private.h:36-60
  declares; the operators call them first and fall back to their CPU code when
  NULL / MagickFalse comes back (e.g. BlurImage, MagickCore/effect.c:783-787;
  ResizeImage, resize.c:3818-3826; EqualizeImage, enhance.c:2072-2075).
  Callers of MagickCore / MagickWand are unchanged.

  The work itself happens behind the C ABI of libmagickhip.so
  (include/magickhip.h), loaded with dlopen on first use (opencl_hip.c): without
  the library, without a GPU, or with the enable switch off every function here
  returns NULL / MagickFalse and the CPU path runs.

  Images stay on the device between chained operators: an operator input is
  uploaded once and its device copy is remembered in CacheInfo::opencl; a result
  is produced on the device and NOT downloaded — the host block is brought up to
  date by the cache hooks in opencl_hip.c the first time the CPU accesses the
  pixels (the reference's own lazy-sync protocol, cache.c:5341-5353).

  Nothing of the reference's OpenCL implementation is used: no cl_mem, no
  kernels-as-strings, no OpenCL runtime.
*/
#include "MagickCore/studio.h"
#include "MagickCore/accelerate-private.h"
#include "MagickCore/cache.h"
#include "MagickCore/cache-private.h"
#include "MagickCore/exception.h"
#include "MagickCore/exception-private.h"
#include "MagickCore/image.h"
#include "MagickCore/image-private.h"
#include "MagickCore/pixel-accessor.h"
#include "MagickCore/resize.h"
#include "MagickCore/resize-private.h"
#include "MagickCore/semaphore.h"
#include "MagickCore/string_.h"
#include "MagickCore/artifact.h"
#include "MagickCore/colorspace.h"
#include "MagickCore/colorspace-private.h"
#include "MagickCore/composite.h"
#include "MagickCore/morphology.h"
#include "MagickCore/profile.h"
#include "MagickCore/property.h"
#include "MagickCore/magick.h"
#include "MagickCore/threshold.h"
#include "MagickCore/geometry.h"

#if defined(MAGICKCORE_OPENCL_SUPPORT)

#include <stdlib.h>
#include "MagickCore/memory_.h"
#include "MagickCore/opencl-private.h"
#include "magickhip_shim.h"

static size_t hip_accelerated_calls=0;        /* read by tests through GetMagickHipAcceleratedCalls */

/* operators run concurrently on different images: the counter is atomic */
#define CountAcceleratedCall() ((void) __atomic_fetch_add(&hip_accelerated_calls,1,__ATOMIC_RELAXED))

MagickExport size_t GetMagickHipAcceleratedCalls(void)
{
  return(__atomic_load_n(&hip_accelerated_calls,__ATOMIC_RELAXED));
}

/*
  `-debug accelerate` (AccelerateEvent, MagickCore/log.h:37-57): which path an operator took.
  Accepted calls name the operator and the image; declined calls say why — the gate that failed
  (the conditions of accelerate.c:110-170), or that the library / the device / the operator
  itself returned "not handled" — and MagickCore then runs its CPU path.
*/
static const char *DescribeGate(const Image *image)
{
  if (image == (const Image *) NULL)
    return("no image");
  if (image->storage_class != DirectClass)
    return("PseudoClass image");
  if ((GetImageArtifact(image,"convolve:bias") != (const char *) NULL) ||
      (GetImageArtifact(image,"convolve:scale") != (const char *) NULL) ||
      (GetImageArtifact(image,"morphology:compose") != (const char *) NULL) ||
      (GetImageArtifact(image,"morphology:showKernel") != (const char *) NULL))
    return("a convolve: / morphology: artifact is set (Blur, UnsharpMask and Convolve hooks decline; "
      "MorphologyApply honours bias, scale and the compose operators None, Lighten, Difference, Darken, Plus, Multiply, Screen, Exclusion, MinusSrc, MinusDst, LinearDodge, Over, DstOver)");
  switch (GetImageVirtualPixelMethod(image))
  {
    case UndefinedVirtualPixelMethod:
    case EdgeVirtualPixelMethod:
      break;
    default:
      return("virtual pixel method other than Undefined / Edge");
  }
  if ((image->channels & (ReadMaskChannel | WriteMaskChannel | CompositeMaskChannel)) != 0)
    return("read, write or composite mask");
  if ((image->number_channels < 1) || (image->number_channels > 4))
    return("more than four channels");
  switch (image->colorspace)
  {
    case RGBColorspace:
    case sRGBColorspace:
    case GRAYColorspace:
    case LinearGRAYColorspace:
      break;
    default:
      return("colourspace outside sRGB / RGB / GRAY / LinearGRAY (or channel layout, artifacts, device, operator arguments)");
  }
  return("channel layout, artifacts, device or operator arguments outside the backend's reach");
}

static void LogAccelerated(const char *function,const Image *image)
{
  if (IsEventLogging() != MagickFalse)
    (void) LogMagickEvent(AccelerateEvent,GetMagickModule(),
      "%s: accelerated on the HIP backend (%.20gx%.20g, %.20g channels, %s)",function,
      (double) image->columns,(double) image->rows,(double) image->number_channels,
      image->filename);
}

static void LogDeclined(const char *function,const int line,const Image *image)
{
  if (IsEventLogging() != MagickFalse)
    (void) LogMagickEvent(AccelerateEvent,GetMagickModule(),
      "%s: not accelerated, the CPU path runs (shim line %d: %s)",function,line,DescribeGate(image));
}

#define HipAccepted(image) (CountAcceleratedCall(),LogAccelerated(__func__,(image)))
#define HipDeclined(image,value) (LogDeclined(__func__,__LINE__,(image)),(value))

/* ------------------------------------------------------------------ gates */
/*
  What the backend can take, the same conditions the reference's accelerate
  layer imposes (accelerate.c:110-170): DirectClass; sRGB / RGB / GRAY /
  LinearGRAY; Undefined or Edge virtual pixels; no read, write or composite
  mask; at most four channels laid out R[,G,B][,A].
*/
static MagickBooleanType IsLayoutAcceleratable(const Image *image);
static MagickBooleanType IsHistogramOperatorAcceleratable(const Image *image);

static MagickBooleanType IsImageAcceleratable(const Image *image)
{
  switch (image->colorspace)
  {
    case RGBColorspace:
    case sRGBColorspace:
    case GRAYColorspace:
    case LinearGRAYColorspace:
      break;
    default:
      return(MagickFalse);
  }
  return(IsLayoutAcceleratable(image));
}

/*
  The gate without the colourspace condition, for the colourspace transform itself and
  for the histogram operators on its result ("the colourspace gate must be
  relaxed for our Lab/linear hooks"; BASELINE config C4 is sRGB->Lab + ContrastStretch).
*/
static MagickBooleanType IsLayoutAcceleratable(const Image *image)
{
  if (image->storage_class != DirectClass)
    return(MagickFalse);
  switch (GetImageVirtualPixelMethod(image))
  {
    case UndefinedVirtualPixelMethod:
    case EdgeVirtualPixelMethod:
      break;
    default:
      return(MagickFalse);
  }
  if ((image->channels & (ReadMaskChannel | WriteMaskChannel | CompositeMaskChannel)) != 0)
    return(MagickFalse);
  if ((image->number_channels < 1) || (image->number_channels > 4))
    return(MagickFalse);
  if (GetPixelChannelOffset(image,RedPixelChannel) != 0)
    return(MagickFalse);
  if ((image->number_channels == 2) || (image->number_channels == 4))
    if (GetPixelChannelOffset(image,AlphaPixelChannel) != (ssize_t) image->number_channels-1)
      return(MagickFalse);
  if (image->number_channels >= 3)
    if ((GetPixelChannelOffset(image,GreenPixelChannel) != 1) ||
        (GetPixelChannelOffset(image,BluePixelChannel) != 2))
      return(MagickFalse);
  return(MagickTrue);
}

/*
  The pixel cache of an image as a private, materialised memory cache (what
  GetAuthenticOpenCLBuffer requires, cache.c:1259-1291).
*/
static CacheInfo *AcquireHeapCache(const Image *image,ExceptionInfo *exception)
{
  CacheInfo
    *cache_info;

  cache_info=(CacheInfo *) image->cache;
  if ((cache_info->type == UndefinedCache) || (cache_info->reference_count > 1))
    {
      if (SyncImagePixelCache((Image *) image,exception) == MagickFalse)
        return((CacheInfo *) NULL);
      cache_info=(CacheInfo *) image->cache;
    }
  if ((cache_info->type != MemoryCache) || (cache_info->mapped != MagickFalse) ||
      (cache_info->pixels == (Quantum *) NULL))
    return((CacheInfo *) NULL);
  return(cache_info);
}

/*
  The device copy of an image's pixels, and the queue (device + stream) the call runs on.

  upload != 0: an operator input.  Resident already: its own device and stream are retained —
  an image stays where its pixels are, and on the stream that produced them, so a chain of
  operators needs no cross-stream ordering (a device that has been switched off meanwhile,
  SetOpenCLDeviceEnabled: the pixels come back to the host first, then as below).  Not
  resident: the arbitration picks a device and a stream (AcquireHipQueue: RequestOpenCLDevice +
  AcquireOpenCLCommandQueue, opencl.c:3056-3102, :656), the host block is uploaded once.  On
  success the caller owns `queue` and gives it back with ReleaseHipQueue.

  upload == 0: an operator result — allocated on the given queue's device and tagged with its
  stream; the host block is stale until the cache hooks download it (record marked dirty).
*/
static void *AcquireDevicePixels(HipLibrary *library,const Image *image,const int upload,
  HipQueue *queue,ExceptionInfo *exception)
{
  CacheInfo
    *cache_info;

  MagickCLCacheInfo
    info;

  void
    *device_pixels;

  cache_info=AcquireHeapCache(image,exception);
  if (cache_info == (CacheInfo *) NULL)
    return(NULL);
  LockSemaphoreInfo(cache_info->semaphore);
  info=cache_info->opencl;
  if ((info != (MagickCLCacheInfo) NULL) && (upload != 0) &&
      (GetOpenCLDeviceEnabled(info->device) == MagickFalse))
    info=cache_info->opencl=CopyMagickCLCacheInfo(info);     /* back to the host: NULL now */
  if (info != (MagickCLCacheInfo) NULL)
    {
      if (upload != 0)
        RetainHipQueue(info->device,(void *) info->events,queue);
      else
        if (info->device != queue->device)
          {
            /* a result cache that is resident elsewhere: not something this file creates */
            UnlockSemaphoreInfo(cache_info->semaphore);
            return(NULL);
          }
      UnlockSemaphoreInfo(cache_info->semaphore);
      return((void *) info->buffer);            /* resident: no transfer */
    }
  if ((upload != 0) && (AcquireHipQueue(library,queue) == MagickFalse))
    {
      UnlockSemaphoreInfo(cache_info->semaphore);
      return(NULL);
    }
  device_pixels=NULL;
  if (library->DeviceAllocAsync(queue->physical,(size_t) cache_info->length,queue->stream,
        &device_pixels) != MH_OK)
    device_pixels=NULL;
  if ((device_pixels != NULL) && (upload != 0))
    {
      if (library->Upload(queue->physical,device_pixels,cache_info->pixels,
            (size_t) cache_info->length,queue->stream) != MH_OK)
        {
          (void) library->DeviceFreeAsync(queue->physical,device_pixels,queue->stream);
          device_pixels=NULL;
        }
      else
        CountHipTransfer(1);
    }
  if (device_pixels == NULL)
    {
      if (upload != 0)
        ReleaseHipQueue(queue);
      UnlockSemaphoreInfo(cache_info->semaphore);
      return(NULL);
    }
  info=(MagickCLCacheInfo) AcquireCriticalMemory(sizeof(*info));
  (void) memset(info,0,sizeof(*info));
  info->buffer=(cl_mem) device_pixels;
  info->device=queue->device;
  info->events=(cl_event *) queue->stream;      /* the stream the copy is used on */
  info->pixels=cache_info->pixels;
  info->length=cache_info->length;
  info->event_count=upload != 0 ? 0U : 1U;      /* dirty: the device copy is the newer one */
  cache_info->opencl=info;
  UnlockSemaphoreInfo(cache_info->semaphore);
  return(device_pixels);
}

static void MarkDeviceCopyNewer(const Image *image)
{
  CacheInfo *cache_info=(CacheInfo *) image->cache;
  /* the cache hooks read and clear the flag under the same semaphore (CopyOpenCLBuffer) */
  LockSemaphoreInfo(cache_info->semaphore);
  if (cache_info->opencl != (MagickCLCacheInfo) NULL)
    cache_info->opencl->event_count=1U;
  UnlockSemaphoreInfo(cache_info->semaphore);
}

static MagickBooleanType DescribeImage(HipLibrary *library,const Image *image,
  void *device_pixels,const HipQueue *queue,MhImage *description)
{
  ssize_t
    i;

#if (MAGICKCORE_QUANTUM_DEPTH != 16)
  return(MagickFalse);
#endif
  library->InitImage(description,device_pixels,image->columns,image->rows,
    (uint32_t) image->number_channels,image->alpha_trait != UndefinedPixelTrait ? 1 : 0,
#if defined(MAGICKCORE_HDRI_SUPPORT)
    MH_QUANTUM_F32,
#else
    MH_QUANTUM_U16,
#endif
    MH_MEMORY_DEVICE);
  description->device=queue->physical;         /* the device the arbitration chose ... */
  description->stream=queue->stream;           /* ... and the stream of this call */
  for (i=0; i < (ssize_t) image->number_channels; i++)
  {
    PixelChannel channel = GetPixelChannelChannel(image,i);
    description->channel_traits[i]=(uint32_t) GetPixelChannelTraits(image,channel);
  }
  description->alpha_offset=(-1);
  if (image->alpha_trait != UndefinedPixelTrait)
    description->alpha_offset=(int32_t) GetPixelChannelOffset(image,AlphaPixelChannel);
  description->alpha_trait=(uint32_t) image->alpha_trait;
  description->colorspace=(uint32_t) image->colorspace;
  description->intensity=(uint32_t) image->intensity;
  description->channel_mask=(uint32_t) image->channel_mask;
  return(MagickTrue);
}

/*
  One accelerated call.  New-image operators: BeginHipCall(call,image,columns,rows) brings the
  source onto a device (or finds it there), clones the result image (CloneImage with a new
  size: a fresh, uninitialised cache, accelerate.c:239-256) whose pixels live on the same device,
  and describes both; the operator runs on call->source / call->destination; EndHipCall returns
  the result image or, when the library declined, destroys it and returns NULL — the CPU path
  then runs.  In-place operators: columns = rows = 0, no result image; EndHipCall marks the
  device copy as the newer one.
*/
typedef struct _HipCall
{
  HipLibrary
    *library;

  HipQueue
    queue;

  Image
    *result;

  size_t
    spread;              /* > 0: host descriptors, the frame's row bands over that many devices */

  MhImage
    source,
    destination;
} HipCall;

/*
  One big image, every GPU.  The reference hands an operator one device (RequestOpenCLDevice,
  opencl.c:3056-3102), and for a pixel cache that lives on the host that device's link then carries
  the whole frame both ways: 2 x 2.1 GB for a 16384^2 RGBA Q16 frame, 75 ms at 57 GB/s, against 2 ms
  of kernel.  When at least two devices are enabled, the source has no device copy and the frame is
  MAGICK_HIP_SPREAD_BYTES (default 256 MiB) or more, the stencil operators (BlurImage,
  UnsharpMaskImage, MorphologyApply) are called on the HOST blocks with MH_DEVICE_ALL — the library
  cuts the frame into row bands (halo rows recomputed) that go round all devices, uploads, kernels
  and downloads overlapping — and EqualizeImage / ContrastStretchImage go through
  MagickHipShardedImage (one band per device, the 65536 x channels table all-reduced).  The result
  stays on the host: a chain of operators on such an image takes this route at every link.
*/
static size_t HostSpreadDevices(const Image *image)
{
  const char
    *value;

  const CacheInfo
    *cache_info;

  size_t
    devices,
    minimum;

  if (AcquireHipLibrary() == (HipLibrary *) NULL)      /* (loads the library and lists the devices) */
    return(0);
  devices=GetHipSpreadDevices();
  if (devices == 0)
    return(0);
  cache_info=(const CacheInfo *) image->cache;
  if ((cache_info == (const CacheInfo *) NULL) || (cache_info->type != MemoryCache) ||
      (cache_info->mapped != MagickFalse) || (cache_info->pixels == (Quantum *) NULL) ||
      (cache_info->opencl != (MagickCLCacheInfo) NULL))
    return(0);
  minimum=(size_t) 256 << 20;
  value=getenv("MAGICK_HIP_SPREAD_BYTES");
  if (value != (const char *) NULL)
    minimum=(size_t) strtoull(value,(char **) NULL,10);
  if ((size_t) cache_info->length < minimum)
    return(0);
  return(devices);
}

static MagickBooleanType DescribeHostImage(HipLibrary *library,const Image *image,
  ExceptionInfo *exception,MhImage *description)
{
  CacheInfo
    *cache_info;

  HipQueue
    none;

  cache_info=AcquireHeapCache(image,exception);
  if ((cache_info == (CacheInfo *) NULL) || (cache_info->opencl != (MagickCLCacheInfo) NULL))
    return(MagickFalse);
  none.device=(MagickCLDevice) NULL;
  none.physical=(-1);
  none.stream=NULL;
  if (DescribeImage(library,image,(void *) cache_info->pixels,&none,description) == MagickFalse)
    return(MagickFalse);
  description->memory=MH_MEMORY_HOST;
  description->device=MH_DEVICE_ALL;
  description->stream=NULL;
  return(MagickTrue);
}

/* BeginHipCall for the new-image stencil operators: the host-spread form when it applies */
static MagickBooleanType BeginHipStencilCall(HipCall *call,const Image *image,ExceptionInfo *exception);

static MagickBooleanType BeginHipCall(HipCall *call,const Image *image,const size_t columns,
  const size_t rows,ExceptionInfo *exception)
{
  void
    *p,
    *q;

  call->spread=0;
  call->result=(Image *) NULL;
  call->queue.device=(MagickCLDevice) NULL;
  call->library=AcquireHipLibrary();
  if (call->library == (HipLibrary *) NULL)
    return(MagickFalse);
  p=AcquireDevicePixels(call->library,image,1,&call->queue,exception);
  if (p == NULL)
    return(MagickFalse);
  if (DescribeImage(call->library,image,p,&call->queue,&call->source) == MagickFalse)
    {
      ReleaseHipQueue(&call->queue);
      return(MagickFalse);
    }
  if ((columns == 0) || (rows == 0))
    return(MagickTrue);
  call->result=CloneImage(image,columns,rows,MagickTrue,exception);
  if ((call->result != (Image *) NULL) &&
      (SetImageStorageClass(call->result,DirectClass,exception) != MagickFalse))
    {
      q=AcquireDevicePixels(call->library,call->result,0,&call->queue,exception);
      if ((q != NULL) && (DescribeImage(call->library,call->result,q,&call->queue,
            &call->destination) != MagickFalse))
        return(MagickTrue);
    }
  if (call->result != (Image *) NULL)
    call->result=DestroyImage(call->result);
  ReleaseHipQueue(&call->queue);
  return(MagickFalse);
}

static MagickBooleanType BeginHipStencilCall(HipCall *call,const Image *image,ExceptionInfo *exception)
{
  size_t
    devices;

  devices=HostSpreadDevices(image);
  if (devices != 0)
    {
      call->spread=0;
      call->result=(Image *) NULL;
      call->queue.device=(MagickCLDevice) NULL;
      call->library=AcquireHipLibrary();
      if ((call->library != (HipLibrary *) NULL) &&
          (DescribeHostImage(call->library,image,exception,&call->source) != MagickFalse))
        {
          call->result=CloneImage(image,image->columns,image->rows,MagickTrue,exception);
          if ((call->result != (Image *) NULL) &&
              (SetImageStorageClass(call->result,DirectClass,exception) != MagickFalse) &&
              (DescribeHostImage(call->library,call->result,exception,&call->destination) != MagickFalse))
            {
              call->spread=devices;
              return(MagickTrue);
            }
          if (call->result != (Image *) NULL)
            call->result=DestroyImage(call->result);
        }
    }
  return(BeginHipCall(call,image,image->columns,image->rows,exception));
}

/* the result image (new-image operators) or NULL when the library declined */
static Image *EndHipCall(HipCall *call,const MhStatus status)
{
  if ((call->spread != 0) && (status == MH_OK))
    CountHipSpreadCall(call->spread);
  ReleaseHipQueue(&call->queue);
  if ((status != MH_OK) && (call->result != (Image *) NULL))
    call->result=DestroyImage(call->result);
  return(call->result);
}

/*
  BlurImage and UnsharpMaskImage reach MorphologyImage on the CPU path (effect.c:1170 ->
  morphology.c:4164-4206), which honours these artifacts: convolve:bias and convolve:scale
  change the kernel, morphology:compose the way the two kernels' results combine,
  morphology:showKernel prints it.  The Accelerate* entry points sit in front of that code, so
  with any of them set they decline; the CPU BlurImage then arrives at the MorphologyApply hook
  with the scaled kernel and the bias, and is accelerated there.
*/
static MagickBooleanType HasMorphologyArtifacts(const Image *image)
{
  if ((GetImageArtifact(image,"convolve:bias") != (const char *) NULL) ||
      (GetImageArtifact(image,"convolve:scale") != (const char *) NULL) ||
      (GetImageArtifact(image,"morphology:compose") != (const char *) NULL) ||
      (GetImageArtifact(image,"morphology:showKernel") != (const char *) NULL))
    return(MagickTrue);
  return(MagickFalse);
}

/* ------------------------------------------------------------- operators */
/*
  Set by AccelerateKuwaharaImage when it declines: KuwaharaImage's CPU code then starts with
  BlurImage (effect.c:1810) on this thread, and that one call stays on the CPU too - past this
  hook and past the one in the MorphologyApply its ConvolveImage ends in, which clears the mark.
  The operator picks a quadrant by a strict comparison of variances of the blurred frame, so behind
  a blur that is within one level (the default mode's) its result is not the CPU's.
*/
static __thread MagickBooleanType
  kuwahara_blur_on_cpu = MagickFalse;

MagickPrivate Image *AccelerateBlurImage(const Image *image,const double radius,
  const double sigma,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *blur_image;

  assert(image != NULL);
  assert(exception != (ExceptionInfo *) NULL);
  if (kuwahara_blur_on_cpu != MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if ((IsImageAcceleratable(image) == MagickFalse) || (HasMorphologyArtifacts(image) != MagickFalse))
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipStencilCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  blur_image=EndHipCall(&call,call.library->BlurImage(&call.source,&call.destination,radius,sigma));
  if (blur_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  blur_image->type=image->type;      /* as MorphologyPrimitive does, morphology.c:2800 */
  HipAccepted(image);
  return(blur_image);
}

MagickPrivate Image *AccelerateUnsharpMaskImage(const Image *image,
  const double radius,const double sigma,const double gain,const double threshold,
  ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *unsharp_image;

  if ((IsImageAcceleratable(image) == MagickFalse) || (HasMorphologyArtifacts(image) != MagickFalse))
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipStencilCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  unsharp_image=EndHipCall(&call,call.library->UnsharpMaskImage(&call.source,&call.destination,
    radius,sigma,gain,threshold));
  if (unsharp_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  unsharp_image->type=image->type;   /* effect.c:4385 */
  HipAccepted(image);
  return(unsharp_image);
}

static double ReferenceFilterWeight(void *user,double x)
{
  return(GetResizeFilterWeight((const ResizeFilter *) user,x));     /* resize.c:1690 */
}

MagickPrivate Image *AccelerateResizeImage(const Image *image,
  const size_t resizedColumns,const size_t resizedRows,
  const ResizeFilter *resizeFilter,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *resize_image;

  MhResizeFilter
    *filter;

  MhStatus
    status;

  if ((IsImageAcceleratable(image) == MagickFalse) || (resizedColumns == 0) || (resizedRows == 0))
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,resizedColumns,resizedRows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  /* the weights are the reference's own: expert filter:* artifacts included */
  filter=call.library->AcquireResizeFilterFromCallback(ReferenceFilterWeight,
    (void *) resizeFilter,GetResizeFilterSupport(resizeFilter));
  status=MH_BAD_ARGUMENT;
  if (filter != (MhResizeFilter *) NULL)
    {
      status=call.library->ResizeImageWithFilter(&call.source,&call.destination,filter);
      (void) call.library->DestroyResizeFilter(filter);
    }
  resize_image=EndHipCall(&call,status);
  if (resize_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  resize_image->type=image->type;    /* resize.c:3872 */
  HipAccepted(image);
  return(resize_image);
}

/*
  SampleImage and ScaleImage: the shim's own hooks (shim/patch_hooks.py), each in front of the sized
  CloneImage (resize.c:3946, :4158), so behind the same-size early return.  ThumbnailImage
  (resize.c:4591) has none: SampleImage -> ResizeImage(Box) -> ResizeImage all arrive here, and its
  frame stays on the device from the one upload of the source to the download of the thumbnail.
  sample:offset is parsed as the reference parses it (resize.c:3958-3972); an offset outside
  [0, 100] % indexes virtual pixels and stays on the CPU.
*/
MagickPrivate Image *AccelerateSampleImage(const Image *image,const size_t columns,const size_t rows,
  ExceptionInfo *exception)
{
  const char
    *value;

  double
    x_percent,
    y_percent;

  HipCall
    call;

  Image
    *sample_image;

  if ((IsImageAcceleratable(image) == MagickFalse) || (columns == 0) || (rows == 0))
    return(HipDeclined(image,(Image *) NULL));
  x_percent=(-1.0);     /* the default: the mid-point of the sample regions */
  y_percent=(-1.0);
  value=GetImageArtifact(image,"sample:offset");
  if (value != (const char *) NULL)
    {
      GeometryInfo
        geometry_info;

      MagickStatusType
        flags;

      flags=ParseGeometry(value,&geometry_info);
      x_percent=geometry_info.rho;
      y_percent=geometry_info.rho;
      if ((flags & SigmaValue) != 0)
        y_percent=geometry_info.sigma;
      if (!((x_percent >= 0.0) && (x_percent <= 100.0) && (y_percent >= 0.0) && (y_percent <= 100.0)))
        return(HipDeclined(image,(Image *) NULL));
    }
  if (BeginHipCall(&call,image,columns,rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  sample_image=EndHipCall(&call,call.library->SampleImage(&call.source,&call.destination,x_percent,y_percent));
  if (sample_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  sample_image->type=image->type;    /* resize.c:4071 */
  HipAccepted(image);
  return(sample_image);
}

MagickPrivate Image *AccelerateScaleImage(const Image *image,const size_t columns,const size_t rows,
  ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *scale_image;

  if ((IsImageAcceleratable(image) == MagickFalse) || (columns == 0) || (rows == 0))
    return(HipDeclined(image,(Image *) NULL));
  /* the result is DirectClass, as resize.c:4161 makes it (BeginHipCall) */
  if (BeginHipCall(&call,image,columns,rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  scale_image=EndHipCall(&call,call.library->ScaleImage(&call.source,&call.destination));
  if (scale_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  scale_image->type=image->type;     /* resize.c:4532 */
  HipAccepted(image);
  return(scale_image);
}

/* EqualizeImage / ContrastStretchImage of one big host-resident image, in place, one row band per
   device with the histogram table all-reduced (MagickHipShardedImage); MagickFalse: not this case
   (or declined: an all-gray colour image, enhance.c:1586-1588) — the caller goes on as before */
static MagickBooleanType ShardedHistogramOperator(Image *image,const MhOperatorKind kind,
  const double black_point,const double white_point,ExceptionInfo *exception)
{
  HipLibrary
    *library;

  MhImage
    description;

  MhOperator
    op;

  size_t
    devices;

  devices=HostSpreadDevices(image);
  if (devices == 0)
    return(MagickFalse);
  library=AcquireHipLibrary();
  if ((library == (HipLibrary *) NULL) ||
      (DescribeHostImage(library,image,exception,&description) == MagickFalse))
    return(MagickFalse);
  (void) memset(&op,0,sizeof(op));
  op.kind=(uint32_t) kind;
  op.args[0]=black_point;
  op.args[1]=white_point;
  if (library->ShardedImage(&op,1,&description,&description,(int) devices,(MhBatchReport *) NULL) != MH_OK)
    return(MagickFalse);
  CountHipSpreadCall(devices);
  HipAccepted(image);
  return(MagickTrue);
}

MagickPrivate MagickBooleanType AccelerateEqualizeImage(Image *image,
  ExceptionInfo *exception)
{
  HipCall
    call;

  MhStatus
    status;

  if (IsHistogramOperatorAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (ShardedHistogramOperator(image,MH_OP_EQUALIZE,0.0,0.0,exception) != MagickFalse)
    return(MagickTrue);
  if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  status=call.library->EqualizeImage(&call.source);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(MagickTrue);
}

/*
  ContrastStretchImage and EqualizeImage start with IdentifyImageType (enhance.c:1586-1588):
  for every sRGB-compatible colourspace an all-gray colour image is first re-laid-out as a GRAY
  image.  The library runs that scan for sRGB and RGB (and hands an all-gray image back to the
  CPU path); the other compatible colourspaces (Adobe98, DisplayP3, ProPhoto, scRGB,
  Transparent) therefore stay on the CPU.  Lab / XYZ (BASELINE config C4) are not
  sRGB-compatible: no scan, accelerated.
*/
static MagickBooleanType IsHistogramOperatorAcceleratable(const Image *image)
{
  switch (image->colorspace)
  {
    case sRGBColorspace:
    case RGBColorspace:
    case GRAYColorspace:
    case LinearGRAYColorspace:
    case LabColorspace:
    case XYZColorspace:
      break;
    default:
      return(HipDeclined(image,MagickFalse));
  }
  return(IsLayoutAcceleratable(image));
}

MagickPrivate MagickBooleanType AccelerateContrastStretchImage(Image *image,
  const double black_point,const double white_point,ExceptionInfo *exception)
{
  HipCall
    call;

  int
    became_gray;

  MhStatus
    status;

  if (IsHistogramOperatorAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (ShardedHistogramOperator(image,MH_OP_CONTRAST_STRETCH,black_point,white_point,exception) != MagickFalse)
    return(MagickTrue);
  if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  became_gray=0;
  status=call.library->ContrastStretchImage(&call.source,black_point,white_point,&became_gray);
  (void) EndHipCall(&call,status);
  /* (an all-gray colour image comes back as MH_UNSUPPORTED: the CPU path then does the
     IdentifyImageType re-layout itself, enhance.c:1586-1588) */
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(MagickTrue);
}

/*
  MorphologyApply (morphology.c:3634): every caller of MorphologyImage / ConvolveImage
  (GaussianBlur, Sharpen, Edge, Emboss, -morphology ...) arrives here through the hook
  shim/patch_hooks.py adds at the top of the reference function.  The KernelInfo list is
  described in place — MhKernelInfo points at the reference's own value arrays.
*/
#define MaxAcceleratedKernels  64

MagickPrivate Image *AccelerateMorphologyApply(const Image *image,
  const MorphologyMethod method,const ssize_t iterations,const KernelInfo *kernel,
  const CompositeOperator compose,const double bias,ExceptionInfo *exception)
{
  const KernelInfo
    *k;

  HipCall
    call;

  Image
    *morphology_image;

  MhKernelInfo
    kernels[MaxAcceleratedKernels];

  MhMorphologyCompose
    override;

  size_t
    n;

  if (kuwahara_blur_on_cpu != MagickFalse)
    {
      kuwahara_blur_on_cpu=MagickFalse;      /* the BlurImage of a declined KuwaharaImage */
      return(HipDeclined(image,(Image *) NULL));
    }
  /* the user's morphology:compose (morphology.c:4206): the operators the backend composes with */
  switch (compose)
  {
    case UndefinedCompositeOp: override=MH_MORPHOLOGY_COMPOSE_DEFAULT; break;
    case NoCompositeOp: override=MH_MORPHOLOGY_COMPOSE_NONE; break;
    case LightenCompositeOp: override=MH_MORPHOLOGY_COMPOSE_LIGHTEN; break;
    case DifferenceCompositeOp: override=MH_MORPHOLOGY_COMPOSE_DIFFERENCE; break;
    case DarkenCompositeOp: override=MH_MORPHOLOGY_COMPOSE_DARKEN; break;
    case PlusCompositeOp: override=MH_MORPHOLOGY_COMPOSE_PLUS; break;
    case MultiplyCompositeOp: override=MH_MORPHOLOGY_COMPOSE_MULTIPLY; break;
    case ScreenCompositeOp: override=MH_MORPHOLOGY_COMPOSE_SCREEN; break;
    case ExclusionCompositeOp: override=MH_MORPHOLOGY_COMPOSE_EXCLUSION; break;
    case MinusSrcCompositeOp: override=MH_MORPHOLOGY_COMPOSE_MINUS_SRC; break;
    case MinusDstCompositeOp: override=MH_MORPHOLOGY_COMPOSE_MINUS_DST; break;
    case LinearDodgeCompositeOp: override=MH_MORPHOLOGY_COMPOSE_LINEAR_DODGE; break;
    case OverCompositeOp: case SrcOverCompositeOp:                        /* both run CompositeOverImage, composite.c:1489 */
      override=MH_MORPHOLOGY_COMPOSE_OVER; break;
    case DstOverCompositeOp: override=MH_MORPHOLOGY_COMPOSE_DST_OVER; break;
    default: return(HipDeclined(image,(Image *) NULL));
  }
  if ((iterations == 0) || (IsImageAcceleratable(image) == MagickFalse))
    return(HipDeclined(image,(Image *) NULL));
  /* CompositeImage's own switches (composite.c:1530-1536): the backend composes with synchronised
     channels and ClampPixel, the defaults */
  if ((GetImageArtifact(image,"compose:sync") != (const char *) NULL) ||
      (GetImageArtifact(image,"compose:clamp") != (const char *) NULL))
    return(HipDeclined(image,(Image *) NULL));
  n=0;
  for (k=kernel; k != (const KernelInfo *) NULL; k=k->next)
  {
    if (n == MaxAcceleratedKernels)
      return(HipDeclined(image,(Image *) NULL));
    (void) memset(&kernels[n],0,sizeof(kernels[n]));
    kernels[n].type=MH_KERNEL_USERDEFINED;
    kernels[n].width=k->width;
    kernels[n].height=k->height;
    kernels[n].x=k->x;
    kernels[n].y=k->y;
    kernels[n].values=(double *) k->values;          /* MagickRealType is double */
    kernels[n].minimum=k->minimum;
    kernels[n].maximum=k->maximum;
    kernels[n].negative_range=k->negative_range;
    kernels[n].positive_range=k->positive_range;
    kernels[n].angle=k->angle;
    if (n != 0)
      kernels[n-1].next=&kernels[n];
    n++;
  }
  if (BeginHipStencilCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  /* MorphologyMethod and MhMorphologyMethod share their values (morphology.h:72-98) */
  morphology_image=EndHipCall(&call,call.library->MorphologyImageCompose(&call.source,
    &call.destination,(MhMorphologyMethod) method,iterations,kernels,bias,override));
  if (morphology_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  morphology_image->type=image->type;                /* morphology.c:2800, :3222 */
  HipAccepted(image);
  return(morphology_image);
}

/*
  TransformImageColorspace (colorspace.c:1751) between sRGB, linear RGB, XYZ and Lab with
  the default illuminant.  The bookkeeping the CPU path does around the pixel loop is
  kept: X -> sRGB ends in SetImageColorspace(sRGB), sRGB -> Y in SetImageColorspace(Y)
  (colorspace.c:1052, :2390).
*/
static MagickBooleanType IsColorspaceAccelerated(const ColorspaceType colorspace)
{
  /* sRGB, linear RGB and the pointwise colourspaces of ConvertRGBToGeneric /
     ConvertGenericToRGB (colorspace.c:958-985, :2292-2319) */
  switch (colorspace)
  {
    case sRGBColorspace: case RGBColorspace: case XYZColorspace: case LabColorspace:
    case CMYColorspace: case HCLColorspace: case HCLpColorspace: case HSBColorspace:
    case HSIColorspace: case HSLColorspace: case HSVColorspace: case HWBColorspace:
    case LCHColorspace: case LCHabColorspace: case LCHuvColorspace: case LMSColorspace:
    case LuvColorspace: case xyYColorspace: case YCbCrColorspace: case YDbDrColorspace:
    case YIQColorspace: case YPbPrColorspace: case YUVColorspace: case JzazbzColorspace:
    case DisplayP3Colorspace: case Adobe98Colorspace: case ProPhotoColorspace:
    case OklabColorspace: case OklchColorspace: case CAT02LMSColorspace:
    /* ... and the table-driven ones (colorspace.c:1254-1420, :2591-2790; YCC as a source is
       declined by the library: its way back goes through YCCMap) */
    case OHTAColorspace: case Rec601YCbCrColorspace: case Rec709YCbCrColorspace: case YCCColorspace:
    case scRGBColorspace: case LogColorspace:
      return(MagickTrue);
    default:
      break;
  }
  return(MagickFalse);
}

/*
  SetImageColorspace for an image whose current pixels live on the device.  It ends in
  SyncImagePixelCache -> GetImagePixelCache, which (a) brings the host block up to date
  (CopyOpenCLBuffer, cache.c:1711) and (b) re-opens a cache whose recorded colourspace
  differs from the image's: a new host block plus a copy of the old one (cache.c:3746-3790).
  Neither is wanted — the pixels are already in the new colourspace and nobody asked for
  them on the host — so the cache is re-tagged first and the device record is set aside for
  the duration of the call.  Should the cache have been replaced all the same, the device
  copy is downloaded into the new block.
*/
static MagickBooleanType SetResidentImageColorspace(HipLibrary *library,Image *image,
  const ColorspaceType colorspace,ExceptionInfo *exception)
{
  CacheInfo
    *cache_info;

  MagickBooleanType
    status;

  MagickCLCacheInfo
    info;

  cache_info=(CacheInfo *) image->cache;
  LockSemaphoreInfo(cache_info->semaphore);
  info=cache_info->opencl;
  cache_info->opencl=(MagickCLCacheInfo) NULL;
  cache_info->colorspace=colorspace;
  UnlockSemaphoreInfo(cache_info->semaphore);
  status=SetImageColorspace(image,colorspace,exception);
  if (info == (MagickCLCacheInfo) NULL)
    return(status);
  cache_info=(CacheInfo *) image->cache;
  LockSemaphoreInfo(cache_info->semaphore);
  if ((cache_info->type == MemoryCache) && (cache_info->pixels == info->pixels) &&
      (cache_info->length == info->length) && (cache_info->opencl == (MagickCLCacheInfo) NULL))
    cache_info->opencl=info;
  else
    {
      const int physical=GetHipDevicePhysical(info->device);
      if ((cache_info->type == MemoryCache) && (cache_info->pixels != (Quantum *) NULL) &&
          (cache_info->length == info->length))
        {
          if (library->Download(physical,cache_info->pixels,(const void *) info->buffer,
                (size_t) info->length,(void *) info->events) != MH_OK)
            status=MagickFalse;
          CountHipTransfer(0);
        }
      else
        status=MagickFalse;
      (void) library->DeviceFreeAsync(physical,(void *) info->buffer,(void *) info->events);
      info=(MagickCLCacheInfo) RelinquishMagickMemory(info);
    }
  UnlockSemaphoreInfo(cache_info->semaphore);
  return(status);
}

/*
  Set by AccelerateCLAHEImage when it declines an image outside Lab: CLAHEImage's CPU code then
  calls TransformImageColorspace twice on this thread (enhance.c:685, :782), and those two calls
  stay on the CPU too.  One level of L (the default mode's conversion is within one) across a bin
  boundary moves the equalised value by a whole bin step.
*/
static __thread int
  clahe_transforms_on_cpu = 0;

MagickPrivate MagickBooleanType AccelerateTransformImageColorspace(Image *image,
  const ColorspaceType colorspace,ExceptionInfo *exception)
{
  HipCall
    call;

  MhStatus
    status;

  if (clahe_transforms_on_cpu > 0)
    {
      clahe_transforms_on_cpu--;
      return(HipDeclined(image,MagickFalse));
    }
  if (((colorspace == GRAYColorspace) || (colorspace == LinearGRAYColorspace)) &&
      (image->colorspace == sRGBColorspace) && (image->number_channels >= 3) &&
      (IsLayoutAcceleratable(image) != MagickFalse))
    {
      /*
        sRGB -> GRAY / LinearGRAY (colorspace.c:843-957): the gray value into the first channel
        on the device; SetImageColorspace then re-lays the pixel cache out as one gray channel
        (it finds the device copy newer and fetches it first: CopyOpenCLBuffer, cache.c:1711) —
        the same hand-over as after AccelerateGrayscaleImage (enhance.c:2500-2510).
      */
      if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
        return(HipDeclined(image,MagickFalse));
      status=call.library->TransformImageColorspace(&call.source,(MhColorspace) colorspace);
      (void) EndHipCall(&call,status);
      if (status != MH_OK)
        return(HipDeclined(image,MagickFalse));
      MarkDeviceCopyNewer(image);
      HipAccepted(image);
      if (SetImageColorspace(image,colorspace,exception) == MagickFalse)
        return(MagickFalse);
      image->type=GrayscaleType;
      return(MagickTrue);
    }
  if ((IsColorspaceAccelerated(image->colorspace) == MagickFalse) ||
      (IsColorspaceAccelerated(colorspace) == MagickFalse) ||
      (image->colorspace == colorspace) || (image->number_channels < 3) ||
      (IsLayoutAcceleratable(image) == MagickFalse) ||
      (GetImageArtifact(image,"color:illuminant") != (const char *) NULL) ||
      (GetImageProperty(image,"white-luminance",exception) != (const char *) NULL))
    return(HipDeclined(image,MagickFalse));          /* D65 and the default Jzazbz white luminance only (colorspace.c:993-995) */
  if (((image->colorspace == LogColorspace) || (colorspace == LogColorspace)) &&
      ((GetImageProperty(image,"gamma",exception) != (const char *) NULL) ||
       (GetImageProperty(image,"film-gamma",exception) != (const char *) NULL) ||
       (GetImageProperty(image,"reference-black",exception) != (const char *) NULL) ||
       (GetImageProperty(image,"reference-white",exception) != (const char *) NULL)))
    return(HipDeclined(image,MagickFalse));          /* the default film parameters only (colorspace.c:1073-1088) */
  if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  /* ColorspaceType and MhColorspace share their values (colorspace.h:27-66) */
  status=call.library->TransformImageColorspace(&call.source,(MhColorspace) colorspace);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(SetResidentImageColorspace(call.library,image,colorspace,exception));
}

/*
  CLAHEImage's call site (the shim's own hook, shim/patch_hooks.py): the top of the function,
  enhance.c:660.  The library converts to Lab, equalises L and converts back in one call, both
  conversions as the bit-identical ones; what AccelerateTransformImageColorspace declines for the
  two transforms is declined here.  The reference reads its padding through the virtual pixels:
  Undefined / Edge only (IsLayoutAcceleratable).  A declined call has touched nothing.
*/
MagickPrivate MagickBooleanType AccelerateCLAHEImage(Image *image,const size_t width,
  const size_t height,const size_t number_bins,const double clip_limit,ExceptionInfo *exception)
{
  const ColorspaceType
    colorspace = image->colorspace;

  HipCall
    call;

  MhStatus
    status;

  /* a declined call keeps its two transforms on the CPU as well (clahe_transforms_on_cpu) */
  clahe_transforms_on_cpu=colorspace != LabColorspace ? 2 : 0;
  if ((image->number_channels < 3) || (IsLayoutAcceleratable(image) == MagickFalse))
    return(HipDeclined(image,MagickFalse));
  if (colorspace != LabColorspace)
    {
      if ((IsColorspaceAccelerated(colorspace) == MagickFalse) ||
          (GetImageArtifact(image,"color:illuminant") != (const char *) NULL) ||
          (GetImageProperty(image,"white-luminance",exception) != (const char *) NULL))
        return(HipDeclined(image,MagickFalse));
      if ((colorspace == LogColorspace) &&
          ((GetImageProperty(image,"gamma",exception) != (const char *) NULL) ||
           (GetImageProperty(image,"film-gamma",exception) != (const char *) NULL) ||
           (GetImageProperty(image,"reference-black",exception) != (const char *) NULL) ||
           (GetImageProperty(image,"reference-white",exception) != (const char *) NULL)))
        return(HipDeclined(image,MagickFalse));
    }
  if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  status=call.library->CLAHEImage(&call.source,width,height,number_bins,clip_limit);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));      /* MH_UNSUPPORTED, MH_BAD_ARGUMENT: the CPU path */
  clahe_transforms_on_cpu=0;
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  if (colorspace == LabColorspace)
    return(MagickTrue);
  /* TransformImageColorspace, colorspace.c:1763-1764 */
  (void) DeleteImageProfile(image,"icc");
  (void) DeleteImageProfile(image,"icm");
  /* what the two SetImageColorspace calls of the transforms leave in the image (gamma, rendering
     intent, chromaticity, type) */
  if (SetResidentImageColorspace(call.library,image,LabColorspace,exception) == MagickFalse)
    return(MagickFalse);
  return(SetResidentImageColorspace(call.library,image,colorspace,exception));
}

/*
  The threshold operators' call sites (the shim's own hooks, shim/patch_hooks.py): the top of
  AdaptiveThresholdImage (threshold.c:216), BilevelImage (:826) and AutoThresholdImage (:691).  The
  library sees the pixels, the traits, the channel mask, the intensity method and the colourspace;
  what it cannot see is gated here: the storage class, a virtual-pixel method other than Undefined
  or Edge (AdaptiveThresholdImage reads its window through the virtual pixels) and the read, write
  and composite masks (IsLayoutAcceleratable).  Any colourspace: the operators compare samples, and
  GetPixelIntensity asks the colourspace only whether it is linear (pixel.c:2356-2455), as the
  library does.  A declined call has touched nothing.
*/
MagickPrivate Image *AccelerateAdaptiveThresholdImage(const Image *image,const size_t width,
  const size_t height,const double bias,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *threshold_image;

  if (IsLayoutAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  threshold_image=EndHipCall(&call,call.library->AdaptiveThresholdImage(&call.source,&call.destination,
    width,height,bias));
  if (threshold_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));      /* a window over the kernels' limits: the CPU path */
  threshold_image->type=image->type;                /* threshold.c:355 */
  HipAccepted(image);
  return(threshold_image);
}

/* BilevelImage retags a frame outside the gray colourspaces as sRGB (threshold.c:828-829) */
static MagickBooleanType RetagThresholdedImage(HipLibrary *library,Image *image,ExceptionInfo *exception)
{
  if ((IsGrayColorspace(image->colorspace) != MagickFalse) || (image->colorspace == sRGBColorspace))
    return(MagickTrue);
  return(SetResidentImageColorspace(library,image,sRGBColorspace,exception));
}

MagickPrivate MagickBooleanType AccelerateBilevelImage(Image *image,const double threshold,
  ExceptionInfo *exception)
{
  HipCall
    call;

  MhStatus
    status;

  if (IsLayoutAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  status=call.library->BilevelImage(&call.source,threshold);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(RetagThresholdedImage(call.library,image,exception));
}

MagickPrivate MagickBooleanType AccelerateAutoThresholdImage(Image *image,
  const AutoThresholdMethod method,ExceptionInfo *exception)
{
  char
    property[MagickPathExtent];

  double
    threshold;

  HipCall
    call;

  MhStatus
    status;

  if (IsLayoutAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (BeginHipCall(&call,image,0,0,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  /* AutoThresholdMethod and MhAutoThresholdMethod share their values (threshold.h:25-31) */
  threshold=0.0;
  status=call.library->AutoThresholdImage(&call.source,(MhAutoThresholdMethod) method,&threshold);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  /* threshold.c:757-760 */
  (void) FormatLocaleString(property,MagickPathExtent,"%g%%",threshold);
  (void) SetImageProperty(image,"auto-threshold:threshold",property,exception);
  if (IsStringTrue(GetImageArtifact(image,"auto-threshold:verbose")) != MagickFalse)
    (void) FormatLocaleFile(stdout,"%.*g%%\n",GetMagickPrecision(),threshold);
  return(RetagThresholdedImage(call.library,image,exception));
}

/*
  The level operators' call sites (the shim's own hooks, shim/patch_hooks.py): the top of LevelImage
  (enhance.c:2938), LevelizeImage (:3092), GammaImage (:2354), NegateImage (:3964),
  SigmoidalContrastImage (:4306), LinearStretchImage (:3375) and MinMaxStretchImage
  (histogram.c:941).  They are pointwise on the samples of the Update channels, in any colourspace;
  what the library cannot see is gated here (IsLayoutAcceleratable: a PseudoClass image has a
  colormap to level too, a masked image pixels to leave alone).  A declined call has touched
  nothing.  NormalizeImage and BrightnessContrastImage need no hook of their own: they reach the
  ContrastStretchImage and FunctionImage ones.
*/
#define BeginLevelsCall(call,image,exception) \
  ((IsLayoutAcceleratable(image) != MagickFalse) && \
   (BeginHipCall((call),(image),0,0,(exception)) != MagickFalse))

static MagickBooleanType EndLevelsCall(HipCall *call,const Image *image,const MhStatus status)
{
  (void) EndHipCall(call,status);
  if (status != MH_OK)
    return(MagickFalse);
  MarkDeviceCopyNewer(image);
  return(MagickTrue);
}

MagickPrivate MagickBooleanType AccelerateLevelImage(Image *image,const double black_point,
  const double white_point,const double gamma,ExceptionInfo *exception)
{
  HipCall
    call;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (EndLevelsCall(&call,image,call.library->LevelImage(&call.source,black_point,white_point,
        gamma)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  return(MagickTrue);
}

MagickPrivate MagickBooleanType AccelerateLevelizeImage(Image *image,const double black_point,
  const double white_point,const double gamma,ExceptionInfo *exception)
{
  HipCall
    call;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (EndLevelsCall(&call,image,call.library->LevelizeImage(&call.source,black_point,white_point,
        gamma)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  return(MagickTrue);
}

/* behind GammaImage's `gamma == 1.0` return; image->gamma as enhance.c:2442-2443 leaves it */
MagickPrivate MagickBooleanType AccelerateGammaImage(Image *image,const double gamma,
  ExceptionInfo *exception)
{
  HipCall
    call;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (EndLevelsCall(&call,image,call.library->GammaImage(&call.source,gamma)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  if (image->gamma != 0.0)
    image->gamma*=gamma;
  return(MagickTrue);
}

MagickPrivate MagickBooleanType AccelerateNegateImage(Image *image,
  const MagickBooleanType grayscale,ExceptionInfo *exception)
{
  HipCall
    call;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (EndLevelsCall(&call,image,call.library->NegateImage(&call.source,
        grayscale != MagickFalse ? 1 : 0)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  return(MagickTrue);
}

/* behind SigmoidalContrastImage's `contrast < MagickEpsilon` return */
MagickPrivate MagickBooleanType AccelerateSigmoidalContrastImage(Image *image,
  const MagickBooleanType sharpen,const double contrast,const double midpoint,
  ExceptionInfo *exception)
{
  HipCall
    call;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (EndLevelsCall(&call,image,call.library->SigmoidalContrastImage(&call.source,
        sharpen != MagickFalse ? 1 : 0,contrast,midpoint)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  return(MagickTrue);
}

/* the range scans, the per-channel order and the LevelImage calls all run in the library */
MagickPrivate MagickBooleanType AccelerateMinMaxStretchImage(Image *image,const double black,
  const double white,const double gamma,ExceptionInfo *exception)
{
  HipCall
    call;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  if (EndLevelsCall(&call,image,call.library->MinMaxStretchImage(&call.source,black,white,
        gamma)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  return(MagickTrue);
}

MagickPrivate MagickBooleanType AccelerateLinearStretchImage(Image *image,
  const double black_point,const double white_point,ExceptionInfo *exception)
{
  char
    property[MagickPathExtent];

  HipCall
    call;

  size_t
    black,
    white;

  if (BeginLevelsCall(&call,image,exception) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  black=0;
  white=0;
  if (EndLevelsCall(&call,image,call.library->LinearStretchImage(&call.source,black_point,
        white_point,&black,&white)) == MagickFalse)
    return(HipDeclined(image,MagickFalse));
  HipAccepted(image);
  /* enhance.c:3423-3425 */
  (void) FormatLocaleString(property,MagickPathExtent,"%gx%g%%",100.0*(ssize_t) black/MaxMap,
    100.0*(ssize_t) white/MaxMap);
  (void) SetImageProperty(image,"histogram:linear-stretch",property,exception);
  return(MagickTrue);
}

/* DespeckleImage's call site: effect.c:1342-1346 */
MagickPrivate Image *AccelerateDespeckleImage(const Image *image,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *despeckle_image;

  if (IsImageAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  despeckle_image=EndHipCall(&call,call.library->DespeckleImage(&call.source,&call.destination));
  if (despeckle_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  despeckle_image->type=image->type;       /* effect.c:1486 */
  HipAccepted(image);
  return(despeckle_image);
}

/* StatisticImage's call site (the shim's own hook, shim/patch_hooks.py): statistic.c:2952 */
MagickPrivate Image *AccelerateStatisticImage(const Image *image,const StatisticType type,
  const size_t width,const size_t height,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *statistic_image;

  if (IsImageAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  /* StatisticType and MhStatisticType share their values (statistic.h:139-152) */
  statistic_image=EndHipCall(&call,call.library->StatisticImage(&call.source,&call.destination,
    (MhStatisticType) type,width,height));
  if (statistic_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  HipAccepted(image);
  return(statistic_image);
}

/* BilateralBlurImage's call site (the shim's own hook, shim/patch_hooks.py): effect.c:935 */
MagickPrivate Image *AccelerateBilateralBlurImage(const Image *image,const size_t width,
  const size_t height,const double intensity_sigma,const double spatial_sigma,
  ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *blur_image;

  /* an even side makes the reference read outside its window: the library declines it too */
  if ((IsImageAcceleratable(image) == MagickFalse) || ((MagickMax(width,1) & 1) == 0) ||
      ((MagickMax(height,1) & 1) == 0))
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  blur_image=EndHipCall(&call,call.library->BilateralBlurImage(&call.source,&call.destination,
    width,height,intensity_sigma,spatial_sigma));
  if (blur_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  blur_image->type=image->type;      /* effect.c:1134 */
  HipAccepted(image);
  return(blur_image);
}

/* SelectiveBlurImage's call site (the shim's own hook, shim/patch_hooks.py): effect.c:3501 */
MagickPrivate Image *AccelerateSelectiveBlurImage(const Image *image,const double radius,
  const double sigma,const double threshold,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *blur_image;

  if (IsImageAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  blur_image=EndHipCall(&call,call.library->SelectiveBlurImage(&call.source,&call.destination,
    radius,sigma,threshold));
  if (blur_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  blur_image->type=image->type;      /* effect.c:3702 */
  HipAccepted(image);
  return(blur_image);
}

/* KuwaharaImage's call site (the shim's own hook, shim/patch_hooks.py): effect.c:1810 */
MagickPrivate Image *AccelerateKuwaharaImage(const Image *image,const double radius,
  const double sigma,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *kuwahara_image;

  /* the library restates the default interpolation, the bilinear branch of
     InterpolatePixelChannels (pixel.c:4975-5033), on edge virtual pixels (the gate's); declined
     calls keep their BlurImage on the CPU as well (kuwahara_blur_on_cpu) */
  kuwahara_blur_on_cpu=MagickTrue;
  if ((IsImageAcceleratable(image) == MagickFalse) || (HasMorphologyArtifacts(image) != MagickFalse) ||
      ((image->interpolate != UndefinedInterpolatePixel) &&
       (image->interpolate != BilinearInterpolatePixel)))
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  kuwahara_image=EndHipCall(&call,call.library->KuwaharaImage(&call.source,&call.destination,
    radius,sigma));
  if (kuwahara_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  kuwahara_blur_on_cpu=MagickFalse;
  HipAccepted(image);
  return(kuwahara_image);
}

/* LocalContrastImage's call site: effect.c:1794-1798 */
MagickPrivate Image *AccelerateLocalContrastImage(const Image *image,const double radius,
  const double strength,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *contrast_image;

  if (IsImageAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  contrast_image=EndHipCall(&call,call.library->LocalContrastImage(&call.source,&call.destination,
    radius,strength));
  if (contrast_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  HipAccepted(image);
  return(contrast_image);
}

/* MotionBlurImage hands its kernel and offsets to the hook (effect.c:2397-2404) */
MagickPrivate Image *AccelerateMotionBlurImage(const Image *image,const double *kernel,
  const size_t width,const OffsetInfo *offset,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *blur_image;

  ptrdiff_t
    *offsets;

  size_t
    i;

  if ((IsImageAcceleratable(image) == MagickFalse) || (width == 0))
    return(HipDeclined(image,(Image *) NULL));
  offsets=(ptrdiff_t *) AcquireQuantumMemory(width,2*sizeof(*offsets));
  if (offsets == (ptrdiff_t *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  for (i=0; i < width; i++)
  {
    offsets[2*i]=(ptrdiff_t) offset[i].x;
    offsets[2*i+1]=(ptrdiff_t) offset[i].y;
  }
  blur_image=(Image *) NULL;
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) != MagickFalse)
    blur_image=EndHipCall(&call,call.library->MotionBlurImageWithKernel(&call.source,
      &call.destination,kernel,width,offsets));
  offsets=(ptrdiff_t *) RelinquishMagickMemory(offsets);
  if (blur_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  HipAccepted(image);
  return(blur_image);
}

/* RotationalBlurImage's call site: effect.c:3241-3245 */
MagickPrivate Image *AccelerateRotationalBlurImage(const Image *image,const double angle,
  ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *blur_image;

  if (IsImageAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  blur_image=EndHipCall(&call,call.library->RotationalBlurImage(&call.source,&call.destination,angle));
  if (blur_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  HipAccepted(image);
  return(blur_image);
}

/*
  WaveletDenoiseImage's own hook (visual-effects.c:3552-3556) does not carry `softness`, on
  which the CPU result depends, so it cannot be honoured; shim/patch_hooks.py redirects the
  call site to the variant below.
*/
MagickPrivate Image *AccelerateWaveletDenoiseImage(const Image *magick_unused(image),
  const double magick_unused(threshold),ExceptionInfo *magick_unused(exception))
{
  return((Image *) NULL);
}

MagickPrivate Image *AccelerateWaveletDenoiseImageSoft(const Image *image,
  const double threshold,const double softness,ExceptionInfo *exception)
{
  HipCall
    call;

  Image
    *noise_image;

  if (IsImageAcceleratable(image) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  if (BeginHipCall(&call,image,image->columns,image->rows,exception) == MagickFalse)
    return(HipDeclined(image,(Image *) NULL));
  noise_image=EndHipCall(&call,call.library->WaveletDenoiseImage(&call.source,&call.destination,
    threshold,softness));
  if (noise_image == (Image *) NULL)
    return(HipDeclined(image,(Image *) NULL));
  HipAccepted(image);
  return(noise_image);
}

MagickPrivate MagickBooleanType AccelerateFunctionImage(Image *image,
  const MagickFunction function,const size_t number_parameters,
  const double *parameters,ExceptionInfo *exception)
{
  HipCall
    call;

  MhStatus
    status;

  if ((image->storage_class != DirectClass) || (IsImageAcceleratable(image) == MagickFalse) ||
      (BeginHipCall(&call,image,0,0,exception) == MagickFalse))
    return(HipDeclined(image,MagickFalse));
  /* MagickFunction and MhFunction share their values (statistic.h:129-136) */
  status=call.library->FunctionImage(&call.source,(MhFunction) function,number_parameters,
    parameters);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(MagickTrue);
}

MagickPrivate MagickBooleanType AccelerateGrayscaleImage(Image *image,
  const PixelIntensityMethod method,ExceptionInfo *exception)
{
  HipCall
    call;

  MhStatus
    status;

  /* only layouts whose first three channels are R,G,B (GrayscaleImage reads all three) */
  if ((image->number_channels < 3) || (IsImageAcceleratable(image) == MagickFalse) ||
      (BeginHipCall(&call,image,0,0,exception) == MagickFalse))
    return(HipDeclined(image,MagickFalse));
  /* PixelIntensityMethod and MhIntensityMethod share their values (pixel.h) */
  status=call.library->GrayscaleImage(&call.source,(MhIntensityMethod) method);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(MagickTrue);       /* the caller sets intensity, type and the GRAY colourspace */
}

/* ContrastImage's call site is live in the reference (enhance.c:1412-1415) */
MagickPrivate MagickBooleanType AccelerateContrastImage(Image *image,
  const MagickBooleanType sharpen,ExceptionInfo *exception)
{
  HipCall
    call;

  MhStatus
    status;

  if ((image->number_channels < 3) || (IsImageAcceleratable(image) == MagickFalse) ||
      (BeginHipCall(&call,image,0,0,exception) == MagickFalse))
    return(HipDeclined(image,MagickFalse));
  status=call.library->ContrastImage(&call.source,sharpen != MagickFalse ? 1 : 0);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(MagickTrue);
}

/*
  ModulateImage's call site (enhance.c:3770-3774) passes the parsed percentages and the
  modulate:colorspace model: all nine models of the reference are taken (HSL is also the
  default for every other value); a color:illuminant artifact (which resets the model and the
  illuminant) is left to the CPU.
*/
MagickPrivate MagickBooleanType AccelerateModulateImage(Image *image,
  const double percent_brightness,const double percent_hue,
  const double percent_saturation,const ColorspaceType colorspace,
  ExceptionInfo *exception)
{
  ColorspaceType
    model;

  HipCall
    call;

  MhStatus
    status;

  /* the nine models of enhance.c:3826-3890; every other value takes ModulateHSL's `default:` */
  switch (colorspace)
  {
    case HCLColorspace: case HCLpColorspace: case HSBColorspace: case HSIColorspace:
    case HSVColorspace: case HWBColorspace: case LCHColorspace: case LCHabColorspace:
    case LCHuvColorspace:
      model=colorspace;
      break;
    default:
      model=HSLColorspace;
      break;
  }
  if ((image->number_channels < 3) || (IsImageAcceleratable(image) == MagickFalse) ||
      (GetImageArtifact(image,"color:illuminant") != (const char *) NULL) ||
      (BeginHipCall(&call,image,0,0,exception) == MagickFalse))
    return(HipDeclined(image,MagickFalse));
  /* ColorspaceType and MhColorspace share their values (colorspace.h:27-66) */
  status=call.library->ModulateImage(&call.source,percent_brightness,percent_saturation,
    percent_hue,(int) model);
  (void) EndHipCall(&call,status);
  if (status != MH_OK)
    return(HipDeclined(image,MagickFalse));
  MarkDeviceCopyNewer(image);
  HipAccepted(image);
  return(MagickTrue);
}

#endif /* MAGICKCORE_OPENCL_SUPPORT */
