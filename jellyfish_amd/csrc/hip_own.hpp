// jellyfish_amd/csrc/hip_own.hpp -- who owns what on the host side of the engine (host only; DESIGN.md, "Host ownership").
// Move-only owners of device memory, pinned memory, streams and events that release in their destructor, the few lines
// every create function and every entry point share, and the two-deep window pipeline under merge and text.  Included by
// jfgpu.hip after HIP_TRY and fail(): every method that can fail returns the JFGPU_* code HIP_TRY would.
// A destructor runs with the handle's device current: the destroy functions set it and drain the streams before `delete`.
// In a handle, streams are declared before the buffers used on them, so the buffers go first.
#pragma once

// Device memory and its capacity in elements.  Growth never keeps the contents unless it says so.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if(this != &o) { (void)reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }
  int reset() {
    T* p = p_; p_ = nullptr; cap_ = 0;
    if(p) HIP_TRY(hipFree(p));
    return JFGPU_OK;
  }
  // exactly n elements, whatever was held before is given up first
  int alloc(size_t n) {
    int rc = reset(); if(rc) return rc;
    HIP_TRY(hipMalloc((void**)&p_, n * sizeof(T)));
    cap_ = n;
    return JFGPU_OK;
  }
  // alloc for callers that carry on without the memory: no error text is set
  bool try_alloc(size_t n) {
    (void)reset();
    if(hipMalloc((void**)&p_, n * sizeof(T)) != hipSuccess) { p_ = nullptr; return false; }
    cap_ = n;
    return true;
  }
  // at least `need` elements: a no-op when they fit, else an eighth more than asked for
  int reserve(size_t need) { return need <= cap_ ? JFGPU_OK : alloc(need + need / 8); }
  // ... a quarter more and 4096, and the first `keep` elements survive (copied on `stream` before the old block goes)
  int reserve_keep(size_t keep, size_t need, hipStream_t stream) {
    if(need <= cap_) return JFGPU_OK;
    DevBuf fresh;
    int rc = fresh.alloc(need + need / 4 + 4096); if(rc) return rc;
    if(keep) HIP_TRY(hipMemcpyAsync(fresh.p_, p_, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    rc = reset(); if(rc) return rc;
    *this = std::move(fresh);
    return JFGPU_OK;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Pinned host memory, the same way.
template <typename T>
class PinBuf {
 public:
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  PinBuf& operator=(PinBuf&& o) noexcept {
    if(this != &o) { (void)reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { (void)reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t cap() const { return cap_; }
  int reset() {
    T* p = p_; p_ = nullptr; cap_ = 0;
    if(p) HIP_TRY(hipHostFree(p));
    return JFGPU_OK;
  }
  int alloc(size_t n) {
    int rc = reset(); if(rc) return rc;
    HIP_TRY(hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault));
    cap_ = n;
    return JFGPU_OK;
  }
  int reserve(size_t need) { return need <= cap_ ? JFGPU_OK : alloc(need + need / 8); }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if(s_ && own_) (void)hipStreamDestroy(s_); }
  int create(unsigned flags = hipStreamNonBlocking) { HIP_TRY(hipStreamCreateWithFlags(&s_, flags)); return JFGPU_OK; }
  void borrow(hipStream_t s) { s_ = s; own_ = false; }               // another handle's stream, which stays that handle's
  hipStream_t get() const { return s_; }
  operator hipStream_t() const { return s_; }
  void sync() const { if(s_) (void)hipStreamSynchronize(s_); }       // before a handle goes

 private:
  hipStream_t s_ = nullptr;
  bool own_ = true;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if(ev_) (void)hipEventDestroy(ev_); }
  int create(unsigned flags = 0) {      // 0: a timing event
    if(flags) HIP_TRY(hipEventCreateWithFlags(&ev_, flags)); else HIP_TRY(hipEventCreate(&ev_));
    return JFGPU_OK;
  }
  hipEvent_t get() const { return ev_; }
  operator hipEvent_t() const { return ev_; }

 private:
  hipEvent_t ev_ = nullptr;
};

// A timed span of launches whose two events go with it (the Bloom counter's profile).
struct OwnedSpan { Event a, b; int which; uint64_t units; };

// The device a create function was asked for (< 0: the current one), made current.
static int pick_device(int requested, int* dev) {
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(JFGPU_E_NO_DEVICE, "no HIP device: the engine has no CPU fallback");
  *dev = requested;
  if(*dev < 0) HIP_TRY(hipGetDevice(dev));
  if(*dev >= ndev) return fail(JFGPU_E_NO_DEVICE, "device ordinal out of range");
  HIP_TRY(hipSetDevice(*dev));
  return JFGPU_OK;
}

// What every entry point of a handle begins with.
template <class H>
int use_dev(const H* h, const char* null_text) {
  if(!h) return fail(JFGPU_E_INVALID, null_text);
  HIP_TRY(hipSetDevice(h->device));
  return JFGPU_OK;
}

static double wall_ms(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// The two-deep pipeline of jfgpu_merge_run, jfgpu_text_run and jfgpu_query_text / jfgpu_bc_query_text: window i is staged in
// pinned memory and uploaded on s_up while the kernels of window i - 1 run on s_k and the output of window i - 2 .. i - 1 is
// downloaded on s_down and sunk.
// A slot (i & 1) is a window's buffers and events.  The callers cut the windows, fill h_in, launch their kernels between
// kernels_begin and kernels_end, and read what their status block means; the steps they share are here.
struct WindowPipe {
  Stream s_up, s_k, s_down;
  struct Slot {
    Event up_a, up_done, ev_a, ev_b, k_done;
    PinBuf<uint8_t> h_in, h_out;                              // pinned staging, in and out
    DevBuf<uint8_t> d_raw, d_out;
    PinBuf<uint8_t> h_status;                                 // what the kernels report of the window: 64-bit words
  } slot[2];
  double ms[4] = {0, 0, 0, 0};                                // upload, kernels, download, sink

  int create(size_t status_bytes) {
    int rc;
    if((rc = s_up.create()) || (rc = s_k.create()) || (rc = s_down.create())) return rc;
    for(Slot& s : slot) {
      if((rc = s.up_a.create()) || (rc = s.up_done.create()) || (rc = s.ev_a.create()) || (rc = s.ev_b.create()) || (rc = s.k_done.create())) return rc;
      if((rc = s.h_status.alloc(status_bytes))) return rc;
    }
    return JFGPU_OK;
  }
  // a run begins: whatever a failed run left behind has ended, the times start at zero
  int begin_run() {
    HIP_TRY(hipStreamSynchronize(s_up)); HIP_TRY(hipStreamSynchronize(s_k)); HIP_TRY(hipStreamSynchronize(s_down));
    for(double& v : ms) v = 0;
    return JFGPU_OK;
  }
  void sync() const { s_up.sync(); s_k.sync(); s_down.sync(); }   // before the handle goes
  // the first `bytes` of the slot's h_in (staged since t0) to d_raw, timed on s_up
  int upload(int i, size_t bytes, std::chrono::steady_clock::time_point t0) {
    Slot& s = slot[i];
    ms[0] += wall_ms(t0);
    HIP_TRY(hipEventRecord(s.up_a, s_up));
    HIP_TRY(hipMemcpyAsync(s.d_raw, s.h_in, bytes, hipMemcpyHostToDevice, s_up));
    HIP_TRY(hipEventRecord(s.up_done, s_up));
    return JFGPU_OK;
  }
  // the kernel span on s_k: after the slot's upload, timed
  int kernels_begin(int i) {
    HIP_TRY(hipStreamWaitEvent(s_k, slot[i].up_done, 0));
    HIP_TRY(hipEventRecord(slot[i].ev_a, s_k));
    return JFGPU_OK;
  }
  int kernels_end(int i) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(slot[i].ev_b, s_k));
    return JFGPU_OK;
  }
  // `bytes` at d_src into the slot's status block from word `at` on, behind the kernels
  int status(int i, size_t at, const void* d_src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(slot[i].h_status + 8 * at, d_src, bytes, hipMemcpyDeviceToHost, s_k));
    return JFGPU_OK;
  }
  const uint64_t* status_words(int i) const { return (const uint64_t*)slot[i].h_status.get(); }
  int done(int i) { HIP_TRY(hipEventRecord(slot[i].k_done, s_k)); return JFGPU_OK; }
  // the slot's kernels and status have arrived; its upload and kernel times are added
  int wait(int i) {
    Slot& s = slot[i];
    HIP_TRY(hipEventSynchronize(s.k_done));
    float t = 0;
    if(hipEventElapsedTime(&t, s.ev_a, s.ev_b) == hipSuccess) ms[1] += t;
    if(hipEventElapsedTime(&t, s.up_a, s.up_done) == hipSuccess) ms[0] += t;
    return JFGPU_OK;
  }
  // the first `bytes` of the slot's d_out into h_out (grown to fit), timed by the wall clock
  int download(int i, size_t bytes) {
    Slot& s = slot[i];
    const auto t0 = std::chrono::steady_clock::now();
    int rc = s.h_out.reserve(bytes); if(rc) return rc;
    HIP_TRY(hipMemcpyAsync(s.h_out, s.d_out, bytes, hipMemcpyDeviceToHost, s_down));
    HIP_TRY(hipStreamSynchronize(s_down));
    ms[2] += wall_ms(t0);
    return JFGPU_OK;
  }
  // the caller's sink, timed when it accepts: its return value
  template <class F>
  int sink(F&& call) {
    const auto t0 = std::chrono::steady_clock::now();
    const int r = call();
    if(!r) ms[3] += wall_ms(t0);
    return r;
  }
};

