// abi_pool_many.inl — what the "many in one call" entry points without a context share (abi_gp_models.inl, abi_pca_models.inl,
// abi_nystrom_models.inl, abi_scan_prep.inl, abi_decimate.inl, abi_samples.inl): the choice of the device, a stream from the pools
// for the length of the call, the list of live items, the repeated argument loops and a kernel term's device record.  The rounds and
// the pieces these calls cut their work into are icp_round_plan.hpp's: index arithmetic without a HIP call.  Every one of them checks
// every item first (live_items), returns if none is left, and only then touches a device (PoolCall).

#include "icp_round_plan.hpp"

namespace {

// the device of a call: `device`, or for a negative one LOCAL_RANK modulo the device count (0 without it)
int resolve_device(int device) {
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    fail(ICP_ERR_DEVICE, std::string("no usable HIP device (this library has no CPU fallback): ") + hipGetErrorString(e));
  if (device < 0) {
    const char* lr = std::getenv("LOCAL_RANK");
    device = lr ? std::atoi(lr) % ndev : 0;
  }
  require(device < ndev, "device ordinal out of range");
  return device;
}

struct DeviceScope {  // the calling thread's device, put back when the call ends
  int prev = -1;
  explicit DeviceScope(int device) {
    (void)hipGetDevice(&prev);
    HIP_OK(hipSetDevice(device));
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
struct StreamScope {
  hipStream_t st;
  explicit StreamScope(int device) : st(take_stream(device, false, 0)) {}
  ~StreamScope() { give_stream(st); }
};
// the device side of a call without a context, from the caller's `device`: behind the validation, in front of the first buffer
struct PoolCall {
  int device;
  DeviceScope bound;
  StreamScope stream;
  hipStream_t st;
  explicit PoolCall(int asked) : device(resolve_device(asked)), bound(device), stream(device), st(stream.st) {}
};

// item_status[b] = ICP_OK where good(b), ICP_ERR_INVALID_ARG elsewhere; returns the good items.  The limits are the entry point's own.
template <class Good>
std::vector<int> live_items(int B, std::vector<int>& item_status, Good good) {
  item_status.assign(B, ICP_OK);
  std::vector<int> live;
  for (int b = 0; b < B; ++b) {
    if (good(b)) live.push_back(b);
    else item_status[b] = ICP_ERR_INVALID_ARG;
  }
  return live;
}

bool all_within(const double* v, size_t n, double max_magnitude) {  // finite (a NaN fails the comparison) and at most that large
  for (size_t i = 0; i < n; ++i)
    if (!(std::fabs(v[i]) <= max_magnitude)) return false;
  return true;
}
bool ids_in_range(const int32_t* ids, size_t n, long long M) {  // every id in [0, M)
  for (size_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= M) return false;
  return true;
}

// the regions of a round's buffer where there are three: the inputs (ONE upload), the work arrays, the outputs (ONE copy back)
enum { kPoolIn, kPoolWork, kPoolOut };

// the device record of a kernel term; device_weights: the term's weights at the points the record is used on, or null
GpmTerm gpm_term_record(const icp_kernel_term_general& k, const double* device_weights) {
  GpmTerm tm{};
  tm.scale = k.scale;
  std::memcpy(tm.A, k.A, sizeof(tm.A));
  tm.kind = k.kind; tm.axis = k.mirror_axis; tm.gain = k.mirror_gain;
  if (k.kind == ICP_KERNEL_GAUSSIAN) tm.sigma2 = k.sigma * k.sigma;
  else tm.c = std::ldexp(1.0, k.level);
  tm.w = device_weights;
  return tm;
}

}  // namespace
