// abi_many.inl — what the batched entry points (abi_*_many.inl, abi_posterior_models.inl) share: the contexts' locks, the argument
// checks, the test hooks' chunk size, coalesced host copies, the packed coefficient upload, the plan of launch_instance_many's records
// and the per-item status epilogue.  Plain functions and small structs; each batched entry point depends on this file and on its own
// kernels only.

namespace {

// every distinct context of a batched call locked, in address order (repeats are allowed: the items of one target share its context);
// returns the distinct contexts
std::vector<icp_ctx*> lock_contexts(int B, icp_ctx* const* ctxs, std::vector<std::unique_lock<std::recursive_mutex>>& locks) {
  std::vector<icp_ctx*> distinct(ctxs, ctxs + B);
  std::sort(distinct.begin(), distinct.end(), std::less<icp_ctx*>());
  distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
  for (icp_ctx* c : distinct) {
    locks.emplace_back(c->mu);
    if (c->batch_busy) fail(ICP_ERR_BUSY, "a context belongs to a batch in flight (icp_chain_step_batched_issue): collect or abandon it first");
  }
  return distinct;
}

void require_one_device(int B, icp_ctx* const* ctxs, const char* text) {
  for (int b = 0; b < B; ++b) require(ctxs[b]->device == ctxs[0]->device, text);
}
void require_one_model(int B, icp_ctx* const* ctxs, const char* text) {
  const icp_ctx& lead = *ctxs[0];
  for (int b = 0; b < B; ++b) {
    const icp_ctx& c = *ctxs[b];
    require(c.device == lead.device && c.r == lead.r && c.N == lead.N && c.Qp.p == lead.Qp.p, text);
  }
}
void require_finite(const double* v, size_t n, const char* text) {
  for (size_t i = 0; i < n; ++i) require(std::isfinite(v[i]), text);
}

// the doubles of an entry point's chunk buffer; test-hooks build: `env_name` gives a small one, so that small meshes take the paths
// of large ones
size_t test_chunk_doubles(const char* env_name, size_t dflt) {
  if (const char* e = dev_env(env_name)) return std::max<size_t>(1, (size_t)std::atoll(e));
  return dflt;
}

// copies between a chunk buffer and the caller's arrays: neighbours on both sides (the rows of one array) go as ONE copy
struct HostCopies {
  struct Run { double* dev; double* host; size_t n; };
  std::vector<Run> runs;
  void add(double* dev, const double* host, size_t n) {
    if (!runs.empty() && runs.back().dev + runs.back().n == dev && runs.back().host + runs.back().n == host) runs.back().n += n;
    else runs.push_back(Run{dev, const_cast<double*>(host), n});
  }
  void issue(hipStream_t st, bool to_device) {
    for (const Run& c : runs) {
      if (to_device) HIP_OK(hipMemcpyAsync(c.dev, c.host, sizeof(double) * c.n, hipMemcpyHostToDevice, st));
      else HIP_OK(hipMemcpyAsync(c.host, c.dev, sizeof(double) * c.n, hipMemcpyDeviceToHost, st));
    }
    runs.clear();
  }
};

// the shape coefficients (theta + 10, r doubles) of a list of states, packed in the list's order and uploaded as ONE copy
struct PackedCoeffs {
  std::vector<double> host;
  explicit PackedCoeffs(size_t doubles) { host.reserve(doubles); }
  void add(const double* theta, int r) { host.insert(host.end(), theta + 10, theta + 10 + r); }
  void upload(DBuf<double>& dst) const {
    NullStreamBatch _nb;
    dst.upload(host.data(), host.size());
  }
};

// the records of launch_instance_many: items in the order they are added, in groups of consecutive items.  A new group opens when
// the model (Qp, N, r) changes, when the open group holds kInstGroup items, or behind boundary() (the start of a round, whose launch
// takes a range of whole groups).  Grouping never changes an item's bits: every item's sums are its own.
struct InstancePlan {
  std::vector<InstanceItem> items;
  std::vector<InstanceGroup> groups;
  bool open = false;
  void boundary() { open = false; }
  void add(const icp_ctx& model, const double* coeffs, const Pose& pose, double* x) {
    if (open && groups.back().Qp == model.Qp.p && groups.back().N == model.N && groups.back().r == model.r && groups.back().n < kInstGroup)
      ++groups.back().n;
    else
      groups.push_back(InstanceGroup{model.Qp.p, model.ref.p, model.mean.p, model.N, model.r, (int)items.size(), 1});
    open = true;
    items.push_back(InstanceItem{coeffs, pose, x});
  }
  void upload(DBuf<InstanceItem>& d_items, DBuf<InstanceGroup>& d_groups) const {
    NullStreamBatch _nb;
    d_items.upload(items.data(), items.size());
    d_groups.upload(groups.data(), groups.size());
  }
};

// the epilogue of a call with per-item statuses: status_out[b] = item_status[b]; returns the first bad code, with text_for(code) as
// the call's error text
int report_item_status(int n, const std::vector<int>& item_status, int32_t* status_out, const char* (*text_for)(int code)) {
  int first_bad = ICP_OK;
  for (int b = 0; b < n; ++b) {
    status_out[b] = item_status[b];
    if (item_status[b] != ICP_OK && first_bad == ICP_OK) {
      first_bad = item_status[b];
      g_err = text_for(first_bad);
    }
  }
  return first_bad;
}

}  // namespace
