// tests/host/own_check.cc -- TEST-ONLY: does the engine's host code give back what it took when an allocation fails?
// The engine's translation unit under the host emulation (-DJFGPU_EMU, as tests/host/build_emu.sh compiles it), in a
// program of its own so that it can be built with -fsanitize=address and run as a plain process (tests/test_own_emu.py).
// The emulation counts device memory in use, live streams and live events, and can make the n-th allocation from now on
// fail (tests/host/hip_emu/hip/hip_runtime.h: fail_alloc_in).
//   creates     for n = 1, 2, ... until the create succeeds: the failed create returned JFGPU_E_ALLOC, handed out no
//               handle and left the three counts where they were; so does destroying the one that succeeded
//   small runs  for every n a run reaches: the run reports an error, destroying its handle brings the counts back, and a
//               fresh handle runs the same job to the result an undisturbed run gave
// At exit LeakSanitizer sees what the counts do not: pinned memory, events, the handles themselves.
#include "../../jellyfish_amd/csrc/jfgpu.hip"

#include <functional>
#include <map>

namespace {

struct Live { size_t mem; long streams, events; };
Live live() { return {hip_emu::mem_in_use(), hip_emu::live_streams(), hip_emu::live_events()}; }
bool same(const Live& a, const Live& b) { return a.mem == b.mem && a.streams == b.streams && a.events == b.events; }

#define CHECK(cond, what)                                                                                              \
  do {                                                                                                                 \
    if(!(cond)) {                                                                                                      \
      const Live l_ = live();                                                                                          \
      fprintf(stderr, "own_check: %s: %s failed at n = %ld (%s:%d); in use now: %zu bytes, %ld streams, %ld events; last error: %s\n", \
              what, #cond, g_n, __FILE__, __LINE__, l_.mem, l_.streams, l_.events, jfgpu_last_error());                \
      exit(1);                                                                                                         \
    }                                                                                                                  \
  } while(0)

long g_n = 0;     // the allocation being failed, for the messages

// runs f with the n-th allocation failing; *fired: it was reached
template <class F>
int with_failure(long n, bool* fired, F&& f) {
  hip_emu::fail_alloc_in() = n;
  const int rc = f();
  *fired = hip_emu::fail_alloc_in() == 0;
  hip_emu::fail_alloc_in() = 0;
  return rc;
}

// create(&handle) -> rc, destroy(handle)
template <class H>
void check_create(const char* what, std::function<int(H**)> create, std::function<void(H*)> destroy) {
  const Live before = live();
  for(g_n = 1;; ++g_n) {
    CHECK(g_n < 1000, what);
    H* h = nullptr;
    bool fired = false;
    const int rc = with_failure(g_n, &fired, [&] { return create(&h); });
    if(!fired) {
      CHECK(rc == JFGPU_OK && h != nullptr, what);
      destroy(h);
      CHECK(same(before, live()), what);
      printf("own_check: %-28s %3ld allocations, each failed once: nothing left behind\n", what, g_n - 1);
      return;
    }
    CHECK(rc == JFGPU_E_ALLOC, what);
    CHECK(h == nullptr, what);
    CHECK(same(before, live()), what);
  }
}

typedef std::vector<uint8_t> Bytes;
void put(Bytes& out, const void* p, size_t n) { out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

// make() -> handle, job(handle, result) -> rc, destroy(handle); check(result): the undisturbed run's result is right;
// every: which allocations are failed -- all of them (1), or the first and every `every`-th after it;
// took_path(handle): after every run that is meant to succeed, the handle shows that the job went the way this check is about;
// absorbed(handle): the job is one the engine may finish without the memory (shards that cannot double carry on as they
// are): a failed allocation may then end without an error, if the handle shows that this is what happened and the result
// is the undisturbed one.  Everything else that returns no error after a failed allocation fails the check.
template <class H>
void check_run(const char* what, std::function<H*()> make, std::function<int(H*, Bytes&)> job, std::function<void(H*)> destroy,
               std::function<bool(const Bytes&)> check, long every = 1, std::function<bool(H*)> took_path = nullptr,
               std::function<bool(H*)> absorbed = nullptr) {
  g_n = 0;
  const Live before = live();
  Bytes ref;
  { H* h = make(); CHECK(h != nullptr, what); CHECK(job(h, ref) == JFGPU_OK, what); CHECK(!took_path || took_path(h), what); destroy(h); }
  CHECK(same(before, live()), what);
  CHECK(check(ref), what);
  long n_absorbed = 0;
  for(g_n = 1;; g_n += every) {
    CHECK(g_n < 1000, what);
    H* h = make(); CHECK(h != nullptr, what);
    Bytes got;
    bool fired = false;
    const int rc = with_failure(g_n, &fired, [&] { return job(h, got); });
    const bool was_absorbed = fired && rc == JFGPU_OK && absorbed && absorbed(h);
    if(!fired) CHECK(!took_path || took_path(h), what);
    destroy(h);
    CHECK(same(before, live()), what);
    if(!fired) {
      CHECK(rc == JFGPU_OK && got == ref, what);
      if(every == 1) printf("own_check: %-28s %3ld allocations, each failed once: error, nothing left behind, a fresh handle is right\n", what, g_n - 1);
      else printf("own_check: %-28s fewer than %ld allocations, every %ld-th failed once: error, nothing left behind, a fresh handle is right\n", what, g_n, every);
      if(absorbed) printf("own_check: %-28s     of them %ld were absorbed: no error, growth off, the undisturbed result\n", what, n_absorbed);
      return;
    }
    if(was_absorbed) { CHECK(got == ref, what); ++n_absorbed; continue; }
    CHECK(rc != JFGPU_OK, what);
    Bytes again;
    h = make(); CHECK(h != nullptr, what);
    CHECK(job(h, again) == JFGPU_OK && again == ref, what);
    CHECK(!took_path || took_path(h), what);
    destroy(h);
    CHECK(same(before, live()), what);
  }
}

// ---- creates ---------------------------------------------------------------------------------------------------------
void table_create(uint32_t k) {
  char what[64]; snprintf(what, sizeof what, "jfgpu_create k = %u", k);
  check_create<jfgpu_table>(what, [k](jfgpu_table** out) {
    jfgpu_params p; memset(&p, 0, sizeof p);
    p.k = k; p.canonical = 1; p.size = 1ull << 20; p.device = -1;
    return jfgpu_create(&p, out);
  }, jfgpu_destroy);
}

void bloom_create_check(uint32_t k, bool filter) {
  char what[64]; snprintf(what, sizeof what, "%s k = %u", filter ? "jfgpu_bf_create" : "jfgpu_bc_create", k);
  check_create<jfgpu_bloom>(what, [k, filter](jfgpu_bloom** out) {
    jfgpu_bloom_params p; memset(&p, 0, sizeof p);
    p.k = k; p.canonical = 1; p.m = 1000003; p.nb_hashes = 3; p.device = -1;
    return filter ? jfgpu_bf_create(&p, out) : jfgpu_bc_create(&p, out);
  }, jfgpu_bc_destroy);
}

// the parser, its upload buffers and the first call that builds its BGZF state: one "create" whose failure takes the
// half-built handle down again
void parser_create_check() {
  check_create<jfgpu_parser>("jfgpu_parser_create + bgzf", [](jfgpu_parser** out) -> int {
    jfgpu_parser* p = nullptr;
    int rc = jfgpu_parser_create(-1, 21, &p);
    if(rc) return rc;
    const char bytes[16] = {0};
    size_t len = 0;
    rc = jfgpu_parser_upload(p, 0, bytes, sizeof bytes);
    if(!rc) rc = jfgpu_parser_inflate_uploaded(p, 0, nullptr, 0, &len);
    if(rc) { jfgpu_parser_destroy(p); return rc; }
    *out = p;
    return JFGPU_OK;
  }, jfgpu_parser_destroy);
}

// ---- small runs --------------------------------------------------------------------------------------------------------
// merge: k = 8 (two key bytes), two-byte counts, 16 positions under the identity matrix (pos = key & 15); position 5 of
// the first input alone is heavier than a window, so the working buffers grow in the middle of the run
constexpr uint32_t kMergeK = 8, kMergeSize = 16, kMergeWindow = 32;
struct MergeInputs { Bytes body[2]; uint64_t n[2] = {0, 0}; std::map<std::pair<uint32_t, uint32_t>, uint64_t> sum; };
MergeInputs merge_inputs() {
  MergeInputs in;
  for(int f = 0; f < 2; ++f)
    for(uint32_t pos = 0; pos < kMergeSize; ++pos) {
      const uint32_t cnt = f == 0 && pos == 5 ? 100 : 10 + pos % 3;
      for(uint32_t j = 0; j < cnt; ++j) {
        const uint32_t key = pos + kMergeSize * (f == 0 ? j : 2 * j + 1);      // ascending inside a position; the inputs share the odd multiples
        const uint16_t val = (uint16_t)(1 + (key * 7 + f) % 50);
        const uint8_t rec[4] = {(uint8_t)key, (uint8_t)(key >> 8), (uint8_t)val, (uint8_t)(val >> 8)};
        put(in.body[f], rec, 4);
        in.sum[{pos, key}] += val;
        ++in.n[f];
      }
    }
  return in;
}
int merge_sink(void* user, const void* bytes, uint64_t n_records) { put(*(Bytes*)user, bytes, (size_t)n_records * 4); return 0; }

void merge_run_check() {
  const MergeInputs in = merge_inputs();
  check_run<jfgpu_merge>("jfgpu_merge_run", [] {
    const uint32_t clen[2] = {2, 2};
    jfgpu_merge_params p; memset(&p, 0, sizeof p);
    p.k = kMergeK; p.n_inputs = 2; p.size = kMergeSize; p.counter_len = clen; p.out_counter_len = 2; p.op = 0;
    p.lower = 0; p.upper = ~0ull; p.device = -1; p.window_records = kMergeWindow;
    jfgpu_merge* m = nullptr;
    return jfgpu_merge_create(&p, &m) == JFGPU_OK ? m : nullptr;
  }, [&in](jfgpu_merge* m, Bytes& out) {
    const void* bodies[2] = {in.body[0].data(), in.body[1].data()};
    int rc = jfgpu_merge_run(m, bodies, in.n, merge_sink, &out);
    uint64_t counts[3] = {0, 0, 0};
    if(!rc) rc = jfgpu_merge_counts(m, counts);
    if(!rc && counts[0] < 3) rc = fail(JFGPU_E_INVALID, "own_check: the merge took fewer than three windows");
    return rc;
  }, jfgpu_merge_destroy, [&in](const Bytes& out) {
    if(out.size() != in.sum.size() * 4) return false;
    size_t i = 0;
    for(const auto& kv : in.sum) {                                             // (position, key) order, counts added
      const uint32_t key = out[4 * i] | (uint32_t)out[4 * i + 1] << 8, val = out[4 * i + 2] | (uint32_t)out[4 * i + 3] << 8;
      if(key != kv.first.second || val != kv.second) return false;
      ++i;
    }
    return true;
  });
}

int text_sink(void* user, const char* text, uint64_t n_bytes, uint64_t) { put(*(Bytes*)user, text, (size_t)n_bytes); return 0; }
void text_run_check() {
  Bytes body;
  const uint32_t n = 160;                                                      // three windows of 64 records
  for(uint32_t i = 0; i < n; ++i) { const uint8_t rec[4] = {(uint8_t)(i * 37), (uint8_t)(i * 11), (uint8_t)(i + 1), 0}; put(body, rec, 4); }
  check_run<jfgpu_text>("jfgpu_text_run", [] {
    jfgpu_text_params p; memset(&p, 0, sizeof p);
    p.k = 8; p.counter_len = 2; p.layout = JFGPU_TEXT_COLUMN; p.separator = ' '; p.lower = 0; p.upper = ~0ull; p.device = -1; p.window_records = 64;
    jfgpu_text* x = nullptr;
    return jfgpu_text_create(&p, &x) == JFGPU_OK ? x : nullptr;
  }, [&body, n](jfgpu_text* x, Bytes& out) {
    int rc = jfgpu_text_run(x, body.data(), n, text_sink, &out);
    uint64_t counts[4] = {0, 0, 0, 0};
    if(!rc) rc = jfgpu_text_counts(x, counts);
    if(!rc && counts[0] != 3) rc = fail(JFGPU_E_INVALID, "own_check: the text run did not take three windows");
    return rc;
  }, jfgpu_text_destroy, [n](const Bytes& out) {
    uint32_t lines = 0;
    for(uint8_t c : out) lines += c == '\n';
    // "KMER COUNT\n": eight bases, a space, the count; the first record counts 1, the last 160
    return lines == n && out.size() > 11 && out[8] == ' ' && out[9] == '1' && out[10] == '\n' && std::string(out.end() - 4, out.end()) == "160\n";
  });
}

// the table's entry points that stage host arrays: add_keys with is_new, lookup, query_ascii
void table_run_check() {
  const uint64_t keys[6] = {1, 2, 3, 0x155555555ull, 2, 77};                    // (2 comes twice)
  const std::string seq = "ACGTTGCAAGGCTTAACCGGTTAACGATCGATTTGACCAGTNACGTACGTTTGACACAGTAGGATCCAT";
  check_run<jfgpu_table>("add_keys / lookup / query", [] {
    jfgpu_params p; memset(&p, 0, sizeof p);
    p.k = 21; p.canonical = 0; p.size = 1ull << 16; p.device = -1;
    jfgpu_table* t = nullptr;
    return jfgpu_create(&p, &t) == JFGPU_OK ? t : nullptr;
  }, [&](jfgpu_table* t, Bytes& out) {
    uint8_t is_new[6] = {9, 9, 9, 9, 9, 9}, found[6] = {9, 9, 9, 9, 9, 9};
    uint64_t vals[6] = {0};
    int rc = jfgpu_add_keys(t, keys, 6, 3, is_new);
    if(!rc) rc = jfgpu_lookup(t, keys, 6, vals, found);
    std::vector<uint64_t> qv(seq.size(), 0); std::vector<uint8_t> qf(seq.size(), 0);
    if(!rc) rc = jfgpu_count_ascii(t, seq.data(), seq.size());
    if(!rc) rc = jfgpu_sync(t);
    if(!rc) rc = jfgpu_query_ascii(t, seq.data(), seq.size(), qv.data(), qf.data());
    put(out, is_new, 6); put(out, found, 6); put(out, vals, sizeof vals); put(out, qv.data(), qv.size() * 8); put(out, qf.data(), qf.size());
    return rc;
  }, jfgpu_destroy, [](const Bytes& out) {
    const uint8_t* is_new = out.data(); const uint8_t* found = out.data() + 6;
    uint64_t vals[6]; memcpy(vals, out.data() + 12, sizeof vals);
    uint64_t q0; memcpy(&q0, out.data() + 12 + sizeof vals + 8 * 20, 8);      // the 21-mer that ends at base 20
    for(int i = 0; i < 6; ++i) if(!found[i] || vals[i] != (i == 1 || i == 4 ? 6u : 3u)) return false;
    return is_new[0] == 1 && is_new[5] == 1 && is_new[1] + is_new[4] == 1 && q0 == 1;     // (the sequence's first 21-mer was counted once)
  });
}

void bloom_run_check() {
  const uint64_t keys[5] = {5, 6, 7, 5, 0x1FFFFFFFFFFull};
  check_run<jfgpu_bloom>("jfgpu_bc_keys", [] {
    jfgpu_bloom_params p; memset(&p, 0, sizeof p);
    p.k = 21; p.canonical = 0; p.m = 100003; p.nb_hashes = 3; p.device = -1;
    jfgpu_bloom* b = nullptr;
    return jfgpu_bc_create(&p, &b) == JFGPU_OK ? b : nullptr;
  }, [&](jfgpu_bloom* b, Bytes& out) {
    uint8_t before[5] = {9, 9, 9, 9, 9}, after[5] = {9, 9, 9, 9, 9};
    int rc = jfgpu_bc_keys(b, keys, 5, before, 1);
    if(!rc) rc = jfgpu_bc_keys(b, keys, 5, after, 0);
    put(out, before, 5); put(out, after, 5);
    return rc;
  }, jfgpu_bc_destroy, [](const Bytes& out) {
    // an insert answers the minimum before it; afterwards 5 was seen twice, the others once
    return out[1] == 0 && out[2] == 0 && out[4] == 0 && out[0] + out[3] == 1 && out[5] == 2 && out[8] == 2 && out[6] == 1 && out[7] == 1 && out[9] == 1;
  });
}

// ---- the communicator, local transport (the one the emulated build has) --------------------------------------------------
// `world` shards of one table, a local communicator over them and a device buffer of input per rank.
struct Shards {
  jfgpu_comm* c = nullptr;
  std::vector<jfgpu_table*> t;
  std::vector<char*> d_in; std::vector<size_t> n;
};
void shards_destroy(Shards* s) {
  jfgpu_comm_destroy(s->c);
  for(jfgpu_table* t : s->t) jfgpu_destroy(t);
  for(char* d : s->d_in) (void)hipFree(d);
  delete s;
}
// rank r's input: bytes[r] random bases (one N in the middle); `items`: JFGPU_COMM_ITEMS, read when the handles are made
Shards* shards_make(int world, uint32_t k, uint64_t size, int mode, const char* items, const std::vector<size_t>& bytes) {
  setenv("JFGPU_COMM_ITEMS", items, 1);
  std::unique_ptr<Shards> s(new Shards);
  uint32_t sb = 0; while((1 << sb) < world) ++sb;
  uint64_t x = 0x2545F4914F6CDD1Dull + world;
  bool ok = true;
  for(int r = 0; r < world && ok; ++r) {
    jfgpu_params p; memset(&p, 0, sizeof p);
    p.k = k; p.canonical = 1; p.size = size; p.device = -1; p.shard_bits = sb; p.shard_id = (uint32_t)r;
    jfgpu_table* t = nullptr;
    ok = jfgpu_create(&p, &t) == JFGPU_OK;
    if(ok) { s->t.push_back(t); ok = !mode || jfgpu_set_mode(t, mode) == JFGPU_OK; }
    std::string seq(bytes[r], 'A');
    for(char& ch : seq) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; ch = "ACGT"[x >> 62]; }
    if(!seq.empty()) seq[seq.size() / 2] = 'N';
    char* d = nullptr;
    ok = ok && hipMalloc((void**)&d, seq.size() + 64) == hipSuccess;
    if(ok) { s->d_in.push_back(d); s->n.push_back(seq.size()); ok = seq.empty() || hipMemcpy(d, seq.data(), seq.size(), hipMemcpyHostToDevice) == hipSuccess; }
  }
  ok = ok && jfgpu_comm_create_local(world, -1, &s->c) == JFGPU_OK;
  Shards* out = s.release();
  if(!ok) { shards_destroy(out); out = nullptr; }
  return out;
}
// one step, the end of the exchange, every shard applied; the result: sent, received and the content of the whole table
// (records, sum of counts, sum and xor of the records' hashes over the shards: whatever the geometry the shards end with)
int shards_step(Shards* s, Bytes& out) {
  uint64_t sent = 0, received = 0, whole[4] = {0, 0, 0, 0};
  int rc = jfgpu_comm_local_step(s->c, s->t.data(), s->d_in.data(), s->n.data());
  if(!rc) rc = jfgpu_comm_finish(s->c, &sent, &received);
  for(jfgpu_table* t : s->t) {
    uint64_t d[4] = {0, 0, 0, 0};
    if(!rc) rc = jfgpu_sync(t);
    if(!rc) rc = jfgpu_digest(t, 0, ~0ull, d);
    whole[0] += d[0]; whole[1] += d[1]; whole[2] += d[2]; whole[3] ^= d[3];
  }
  put(out, &sent, 8); put(out, &received, 8); put(out, whole, sizeof whole);
  return rc;
}
void comm_create_check(int world) {
  char what[64]; snprintf(what, sizeof what, "jfgpu_comm_create_local W = %d", world);
  check_create<jfgpu_comm>(what, [world](jfgpu_comm** out) { return jfgpu_comm_create_local(world, -1, out); }, jfgpu_comm_destroy);
}

// every: only every `every`-th allocation of the run is failed (1: all of them)
void comm_step_check(const char* what, int world, uint32_t k, uint64_t size, int mode, const char* items, const std::vector<size_t>& bytes, long every,
                     std::function<bool(Shards*)> took_path, std::function<bool(Shards*)> absorbed = nullptr) {
  uint64_t mers = 0;                                                           // the N at b / 2 cuts an input in two runs
  for(size_t b : bytes) for(size_t run : {b / 2, b - b / 2 - (b ? 1 : 0)}) mers += run >= k ? run - k + 1 : 0;
  check_run<Shards>(what, [&] { return shards_make(world, k, size, mode, items, bytes); }, shards_step, shards_destroy,
                    [mers](const Bytes& out) {                                 // what was sent arrived, and the table counts every k-mer of the input
    uint64_t v[6]; memcpy(v, out.data(), sizeof v);
    return v[0] == mers && v[1] == mers && v[3] == mers;
  }, every, took_path, absorbed);
}
// how the step just made travelled: every rank's region capacity of that step (0: as keys); as items, every rank was
// also sent some (the claims summed by the receive side)
bool step_went_as_items(Shards* s) {
  for(auto& R : s->c->ranks) {
    unsigned long long claimed = 0;
    if(!R.icap[R.turn ^ 1] || hipMemcpy(&claimed, R.d_claimed, 8, hipMemcpyDeviceToHost) != hipSuccess || !claimed) return false;
  }
  return true;
}
bool step_went_as_keys(Shards* s) {
  for(auto& R : s->c->ranks) if(R.icap[R.turn ^ 1]) return false;
  return true;
}

// two counters filled with different keys, merged: both hold the cells of both
struct Blooms { jfgpu_comm* c = nullptr; jfgpu_bloom* b[2] = {nullptr, nullptr}; };
void blooms_destroy(Blooms* s) { jfgpu_comm_destroy(s->c); for(jfgpu_bloom* b : s->b) jfgpu_bc_destroy(b); delete s; }
void comm_bc_merge_check() {
  check_run<Blooms>("jfgpu_comm_bc_merge_local", [] {
    Blooms* s = new Blooms;
    bool ok = true;
    for(int r = 0; r < 2 && ok; ++r) {
      jfgpu_bloom_params p; memset(&p, 0, sizeof p);
      p.k = 21; p.canonical = 0; p.m = 100003; p.nb_hashes = 3; p.device = -1;
      const uint64_t keys[3] = {5, 6 + (uint64_t)r, 7 + 2 * (uint64_t)r};
      uint8_t before[3];
      ok = jfgpu_bc_create(&p, &s->b[r]) == JFGPU_OK && jfgpu_bc_keys(s->b[r], keys, 3, before, 1) == JFGPU_OK;
    }
    ok = ok && jfgpu_comm_create_local(2, -1, &s->c) == JFGPU_OK;
    if(!ok) { blooms_destroy(s); s = nullptr; }
    return s;
  }, [](Blooms* s, Bytes& out) {
    int rc = jfgpu_comm_bc_merge_local(s->c, s->b);
    const uint64_t keys[5] = {5, 6, 7, 9, 8};                 // seen twice, once, twice (rank 0's 7, rank 1's 7), once, never
    for(jfgpu_bloom* b : s->b) { uint8_t got[5] = {9, 9, 9, 9, 9}; if(!rc) rc = jfgpu_bc_keys(b, keys, 5, got, 0); put(out, got, 5); }
    return rc;
  }, blooms_destroy, [](const Bytes& out) {
    const uint8_t want[5] = {2, 1, 2, 1, 0};
    return out.size() == 10 && !memcmp(out.data(), want, 5) && !memcmp(out.data() + 5, want, 5);
  });
}

}  // namespace

int main() {
  for(uint32_t k : {21u, 40u, 100u}) table_create(k);
  bloom_create_check(21, false); bloom_create_check(100, false); bloom_create_check(21, true);
  parser_create_check();
  check_create<jfgpu_merge>("jfgpu_merge_create", [](jfgpu_merge** out) {
    const uint32_t clen[2] = {2, 4};
    uint64_t cols[16]; for(int i = 0; i < 16; ++i) cols[i] = 1ull << (i % 8);    // any matrix: its byte tables go to the device
    jfgpu_merge_params p; memset(&p, 0, sizeof p);
    p.k = 8; p.n_inputs = 2; p.size = 256; p.matrix_columns = cols; p.counter_len = clen; p.out_counter_len = 2; p.upper = ~0ull; p.device = -1;
    return jfgpu_merge_create(&p, out);
  }, jfgpu_merge_destroy);
  check_create<jfgpu_text>("jfgpu_text_create", [](jfgpu_text** out) {
    jfgpu_text_params p; memset(&p, 0, sizeof p);
    p.k = 21; p.counter_len = 4; p.layout = JFGPU_TEXT_FASTA; p.upper = ~0ull; p.device = -1;
    return jfgpu_text_create(&p, out);
  }, jfgpu_text_destroy);
  merge_run_check();
  text_run_check();
  table_run_check();
  bloom_run_check();
  comm_create_check(2); comm_create_check(4);
  comm_step_check("comm step, keys", 2, 16, 1ull << 20, 2, "0", {90000, 40000}, 1, step_went_as_keys);
  // a shape of test_comm_item_path_equals_single_table (k = 16, world 2, 2^26 slots, partitioned mode: a shard has its two
  // partition levels, which the item path needs); steps of 90000 and 40000 bytes
  comm_step_check("comm step, items", 2, 16, 1ull << 26, 2, "2", {90000, 40000}, 1, step_went_as_items);
  // shards of 2^11 slots for 10^5 distinct k-mers: the first step doubles them, more than once.  A doubled shard that cannot
  // be allocated is no error (comm_grow: "if anybody cannot, nobody grows"): growth goes off on every shard
  comm_step_check("comm step, comm_grow", 2, 21, 1ull << 12, 0, "0", {60000, 20000}, 1, [](Shards* s) {
    jfgpu_info a, b;
    return jfgpu_get_info(s->t[0], &a) == JFGPU_OK && jfgpu_get_info(s->t[1], &b) == JFGPU_OK && a.lsize > 15 && a.lsize == b.lsize;
  }, [](Shards* s) { return !s->t[0]->grow_on && !s->t[1]->grow_on; });
  comm_bc_merge_check();
  const Live end = live();
  if(end.mem || end.streams || end.events) { fprintf(stderr, "own_check: at exit %zu bytes, %ld streams, %ld events are still held\n", end.mem, end.streams, end.events); return 1; }
  printf("own_check: ok\n");
  return 0;
}
