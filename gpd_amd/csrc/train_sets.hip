// The trainer's two resident image sets (0: training, 1: test): pools on the device that are set, reserved, appended
// to from the host or straight from a labelled view, read back and reordered in place.  A pool holds cap >= n images of
// 3600 C bytes and their labels; the passes (train_passes.hip) read the first n through index lists.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "context.h"
#include "buffers.h"
#include "train.h"

using namespace gpd;

namespace {

// gpd_hip_train_reorder: image k of the range = image order[k] of its copy in the scratch block, in 16-byte units (one per
// lane: dwordx4 loads and stores) as label.hip's gather moves them; the label rides along on the first lane
__global__ void __launch_bounds__(256) pool_reorder_kernel(const uint4 *__restrict__ src, const uint8_t *__restrict__ src_labels,
                                                           const int32_t *__restrict__ order, uint4 *__restrict__ dst,
                                                           uint8_t *__restrict__ dst_labels, unsigned img_units, unsigned blocks_per) {
  const unsigned k = blockIdx.x / blocks_per, b = blockIdx.x - k * blocks_per;
  const unsigned u = b * 256 + threadIdx.x;
  const size_t from = (size_t)order[k];
  if (u < img_units) dst[(size_t)k * img_units + u] = src[from * img_units + u];
  if (u == 0) dst_labels[k] = src_labels[from];
}

size_t image_bytes(const gpd_hip_trainer *t) { return (size_t)kPix * t->p.channels; }

// pool `which` holds exactly `capacity` (>= n) images afterwards, its first n kept.  The stream is synchronised before a pool is
// moved or freed; a failed allocation is GPD_ERR_CAPACITY and leaves the pool as it was
int pool_resize(const char *who, gpd_hip_trainer *t, int which, int capacity) {
  if (capacity == t->cap[which]) return GPD_OK;
  const size_t ib = image_bytes(t);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipStreamSynchronize(t->stream));
  uint8_t *img = nullptr, *lab = nullptr;
  if (capacity > 0) {
    hipError_t e = device_alloc(img, (size_t)capacity * ib);
    if (e == hipSuccess) e = device_alloc(lab, (size_t)capacity);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      device_release(img);
      set_error("%s: no room for %d images of %d channels (%zu bytes): %s", who, capacity, t->p.channels, (size_t)capacity * (ib + 1),
                hipGetErrorString(e));
      return GPD_ERR_CAPACITY;
    }
    if (t->n[which] > 0) {
      hipError_t c = hipMemcpyAsync(img, t->d_img[which], (size_t)t->n[which] * ib, hipMemcpyDeviceToDevice, t->stream);
      if (c == hipSuccess) c = hipMemcpyAsync(lab, t->d_lab[which], (size_t)t->n[which], hipMemcpyDeviceToDevice, t->stream);
      if (c == hipSuccess) c = hipStreamSynchronize(t->stream);
      if (c != hipSuccess) {
        device_release(img, lab);
        set_error("%s: moving the pool failed: %s", who, hipGetErrorString(c));
        return GPD_ERR_HIP;
      }
    }
  }
  device_release(t->d_img[which], t->d_lab[which]);
  t->d_img[which] = img;
  t->d_lab[which] = lab;
  t->cap[which] = capacity;
  return GPD_OK;
}

// room for `more` images behind n: geometric growth, at least x 1.5 and never less than the need
int pool_grow(const char *who, gpd_hip_trainer *t, int which, long long more) {
  const long long need = (long long)t->n[which] + more;
  if (need > 0x7fffffffll) {
    set_error("%s: %lld images, a resident set counts them in an int", who, need);
    return GPD_ERR_CAPACITY;
  }
  if (need <= t->cap[which]) return GPD_OK;
  const long long grown = (long long)t->cap[which] + t->cap[which] / 2 + 1;
  return pool_resize(who, t, which, (int)std::min(std::max(need, grown), 0x7fffffffll));
}

int check_labels(const char *who, const uint8_t *labels, int n) {
  for (int i = 0; i < n; i++)
    if (labels[i] > 1) return invalid("%s: label %d of image %d (0 or 1)", who, (int)labels[i], i);
  return GPD_OK;
}

// host images and labels, n > 0 of them, behind image `at` of pool `which`, which has the room; waited for
int upload_images(gpd_hip_trainer *t, int which, size_t at, const uint8_t *images_hwc, const uint8_t *labels, int n) {
  const size_t ib = image_bytes(t);
  HIP_RET(hipMemcpyAsync(t->d_img[which] + at * ib, images_hwc, (size_t)n * ib, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipMemcpyAsync(t->d_lab[which] + at, labels, (size_t)n, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  return GPD_OK;
}

// gpd_hip_train_append_view's sink: the pool grows when the view's kept count is known, the gather writes behind n
struct ViewSink {
  gpd_hip_trainer *t;
  int which;
  static int place(void *self, size_t k, uint8_t **images, uint8_t **labels) {
    ViewSink *s = static_cast<ViewSink *>(self);
    const int rc = pool_grow("gpd_hip_train_append_view", s->t, s->which, (long long)k);
    if (rc) return rc;
    *images = s->t->d_img[s->which] + (size_t)s->t->n[s->which] * image_bytes(s->t);
    *labels = s->t->d_lab[s->which] + (size_t)s->t->n[s->which];
    return GPD_OK;
  }
};

}  // namespace

extern "C" {

// not pool_resize: the old pool goes before the new one is allocated (a set near the device's memory can be replaced), the new
// one holds exactly n, and a set above 4 GiB is refused
int gpd_hip_train_set_data(gpd_hip_trainer *t, int which, const uint8_t *images_hwc, const uint8_t *labels, int n) {
  if (!set_ok(t, which) || n < 0 || (n > 0 && (!images_hwc || !labels))) return invalid("gpd_hip_train_set_data: bad argument");
  const int rc = check_labels("gpd_hip_train_set_data", labels, n);
  if (rc) return rc;
  const size_t bytes = (size_t)n * image_bytes(t);
  if (bytes > ((size_t)4 << 30)) {
    set_error("gpd_hip_train_set_data: %d images of %d channels are %zu bytes; a resident set holds 4 GiB", n, t->p.channels, bytes);
    return GPD_ERR_CAPACITY;
  }
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipStreamSynchronize(t->stream));
  device_release(t->d_img[which], t->d_lab[which]);
  t->n[which] = t->cap[which] = 0;
  if (n == 0) return GPD_OK;
  HIP_RET(device_alloc(t->d_img[which], bytes));
  HIP_RET(device_alloc(t->d_lab[which], (size_t)n));
  const int up = upload_images(t, which, 0, images_hwc, labels, n);
  if (up) return up;
  t->n[which] = t->cap[which] = n;
  return GPD_OK;
}

int gpd_hip_train_reserve(gpd_hip_trainer *t, int which, int capacity_images) {
  if (!set_ok(t, which) || capacity_images < 0) return invalid("gpd_hip_train_reserve: bad argument");
  return pool_resize("gpd_hip_train_reserve", t, which, std::max(capacity_images, t->n[which]));
}

int gpd_hip_train_count(gpd_hip_trainer *t, int which, int *n, int *capacity) {
  if (!set_ok(t, which) || !n) return invalid("gpd_hip_train_count: bad argument");
  *n = t->n[which];
  if (capacity) *capacity = t->cap[which];
  return GPD_OK;
}

int gpd_hip_train_append_data(gpd_hip_trainer *t, int which, const uint8_t *images_hwc, const uint8_t *labels, int n) {
  if (!set_ok(t, which) || n < 0 || (n > 0 && (!images_hwc || !labels))) return invalid("gpd_hip_train_append_data: bad argument");
  int rc = check_labels("gpd_hip_train_append_data", labels, n);
  if (rc) return rc;
  if (n == 0) return GPD_OK;
  HIP_RET(hipSetDevice(t->device));
  rc = pool_grow("gpd_hip_train_append_data", t, which, n);
  if (rc) return rc;
  rc = upload_images(t, which, (size_t)t->n[which], images_hwc, labels, n);
  if (rc) return rc;
  t->n[which] += n;
  return GPD_OK;
}

int gpd_hip_train_get_data(gpd_hip_trainer *t, int which, int first, int count, uint8_t *images_hwc, uint8_t *labels) {
  if (!set_ok(t, which) || first < 0 || count < 0 || (long long)first + count > t->n[which] || (count > 0 && (!images_hwc || !labels)))
    return invalid("gpd_hip_train_get_data: bad argument, or a range outside the %d images of the set", set_ok(t, which) ? t->n[which] : 0);
  if (count == 0) return GPD_OK;
  const size_t ib = image_bytes(t);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(images_hwc, t->d_img[which] + (size_t)first * ib, (size_t)count * ib, hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipMemcpyAsync(labels, t->d_lab[which] + (size_t)first, (size_t)count, hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  return GPD_OK;
}

int gpd_hip_train_reorder(gpd_hip_trainer *t, int which, int first, int count, const int32_t *order) {
  if (!set_ok(t, which) || first < 0 || count < 0 || (long long)first + count > t->n[which] || (count > 0 && !order))
    return invalid("gpd_hip_train_reorder: bad argument, or a range outside the %d images of the set", set_ok(t, which) ? t->n[which] : 0);
  std::vector<uint8_t> seen((size_t)count, 0);
  bool identity = true;
  for (int k = 0; k < count; k++) {
    if (order[k] < 0 || order[k] >= count || seen[(size_t)order[k]])
      return invalid("gpd_hip_train_reorder: order[%d] = %d: not a permutation of 0 .. %d", k, order[k], count - 1);
    seen[(size_t)order[k]] = 1;
    identity = identity && order[k] == k;
  }
  if (identity) return GPD_OK;
  const size_t ib = image_bytes(t);
  const unsigned units = (unsigned)(ib / 16), per = (units + 255) / 256;  // 3600 C bytes: a multiple of 16
  if ((unsigned long long)count * per > 0x7fffffffull) {
    set_error("gpd_hip_train_reorder: %d images are more than one launch takes", count);
    return GPD_ERR_CAPACITY;
  }
  HIP_RET(hipSetDevice(t->device));
  // the scratch block: the range's images | its order | its labels
  const size_t off_order = (size_t)count * ib, off_lab = off_order + ((size_t)count * sizeof(int32_t) + 15) / 16 * 16;
  uint8_t *scratch = nullptr;
  if (device_alloc(scratch, off_lab + (size_t)count) != hipSuccess) {
    (void)hipGetLastError();
    set_error("gpd_hip_train_reorder: no room for a scratch block of %zu bytes", off_lab + (size_t)count);
    return GPD_ERR_CAPACITY;
  }
  uint8_t *img = t->d_img[which] + (size_t)first * ib, *lab = t->d_lab[which] + (size_t)first;
  hipError_t e = hipMemcpyAsync(scratch, img, (size_t)count * ib, hipMemcpyDeviceToDevice, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(scratch + off_lab, lab, (size_t)count, hipMemcpyDeviceToDevice, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(scratch + off_order, order, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pool_reorder_kernel, dim3((unsigned)count * per), dim3(256), 0, t->stream, reinterpret_cast<const uint4 *>(scratch),
                       scratch + off_lab, reinterpret_cast<const int32_t *>(scratch + off_order), reinterpret_cast<uint4 *>(img), lab, units, per);
    e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(t->stream);
  device_release(scratch);
  if (e != hipSuccess || e2 != hipSuccess) {
    set_error("gpd_hip_train_reorder: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return GPD_ERR_HIP;
  }
  return GPD_OK;
}

int gpd_hip_train_append_view(gpd_hip_trainer *t, int which, gpd_hip_ctx *ctx, gpd_label_view_job *job) {
  if (!set_ok(t, which) || !ctx || !job) return invalid("gpd_hip_train_append_view: bad argument");
  if (ctx->device != t->device || ctx->params.image_num_channels != t->p.channels)
    return invalid("gpd_hip_train_append_view: the context is on device %d with %d channels, the trainer on device %d with %d", ctx->device,
                   ctx->params.image_num_channels, t->device, t->p.channels);
  ViewSink vs{t, which};
  const LabelSink sink{&vs, &ViewSink::place};
  const int rc = label_view_run(ctx, job, "gpd_hip_train_append_view", &sink);
  if (rc) return rc;
  t->n[which] += job->num_out;  // label_view_run returned after the gather's event: the next step sees the images
  return GPD_OK;
}

}  // extern "C"
