/* include/jfgpu.h -- C ABI of the MI355X-native k-mer counting engine (libjfgpu.so).
 *
 * This is the drop-in boundary for the `jellyfish count` hot path.  The
 * reference (gmarcais/Jellyfish, /root/reference) has no FFI: its seam is the C++
 * template API `jellyfish::cooperative::hash_counter<mer_dna>` plus the
 * binary/sorted file format.  Each entry point below names the reference
 * interface (file:line relative to /root/reference) it stands in for; the C++
 * facade in jellyfish_amd/include/jellyfish_amd/ and the `jellyfish-amd` CLI sit
 * on top of exactly these functions.
 *
 * Conventions
 *  - plain C: opaque handle, pointers + sizes, int return codes (0 = ok), no
 *    exceptions cross the boundary; jfgpu_last_error() gives the message the
 *    reference would have thrown (e.g. "Hash full", hash_counter.hpp:194-195).
 *  - k-mers are arrays of ceil(k/32) little-endian uint64 words, word 0 least
 *    significant, base i of the string (0 = leftmost) at bits 2(k-1-i), A=0 C=1
 *    G=2 T=3 -- the in-memory layout of mer_dna (mer_dna.hpp:143-155,526-542),
 *    i.e. what mer_dna::data() returns and binary_writer writes.
 *  - buffers are host pointers unless the function name ends in _dev (then the
 *    pointer is device memory on the table's GPU, e.g. a torch tensor's
 *    data_ptr()).  All work is enqueued on the table's HIP stream; functions that
 *    return results to the host synchronise that stream.
 *  - the engine needs a gfx950 GPU.  There is no CPU fallback: every call fails
 *    with JFGPU_E_NO_DEVICE when no HIP device is usable.
 */
#ifndef JFGPU_H
#define JFGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JFGPU_ABI_VERSION 1

enum {
  JFGPU_OK = 0,
  JFGPU_E_INVALID = 1,    /* bad argument (std::length_error / out_of_range in the reference) */
  JFGPU_E_NO_DEVICE = 2,  /* no usable HIP device / kernel image */
  JFGPU_E_ALLOC = 3,      /* large_hash::array::ErrorAllocation, large_hash_array.hpp:55,169-172 */
  JFGPU_E_FULL = 4,       /* std::runtime_error("Hash full"), hash_counter.hpp:194-195 */
  JFGPU_E_HIP = 5,        /* HIP runtime error */
  JFGPU_E_UNSUPPORTED = 6,/* combination not built (e.g. k > 128, a one-pass filter over shards, a filter on a shard of keys of more than two words) */
  JFGPU_E_FORMAT = 7,     /* device parser: chunk is not in the strict layout it handles; give it to the host parser */
  JFGPU_E_CORRUPT = 8     /* compressed input (BGZF / BAM) is malformed or fails its CRC32 / ISIZE check: there is no
                             host path for it, the input is bad (htslib's "bgzf_read" / "truncated file" errors) */
};

typedef struct jfgpu_table jfgpu_table; /* opaque: one hash shard resident in one GPU's HBM */

/* Parameters of a table.  Mirrors the ctor of hash_counter / large_hash::array
 * (hash_counter.hpp:56-64, large_hash_array.hpp:992-1001) minus the CPU-only knobs
 * (nb_threads, reprobe schedule: the in-memory probing is never serialised). */
typedef struct jfgpu_params {
  uint32_t k;            /* mer length; key_len = 2k bits.  1..128 (one to four 64-bit key words; the reference's
                            mer_dna takes any length, mer_dna.hpp:711-717 -- longer is JFGPU_E_UNSUPPORTED here) */
  uint32_t canonical;    /* count_main.cc -C: count min(mer, revcomp) */
  uint64_t size;         /* requested GLOBAL number of slots (hint: rounded up to a power of
                            two, capped at 4^k, raised to the engine minimum for large k) */
  int32_t  device;       /* HIP device ordinal, -1 = current device */
  uint32_t shard_bits;   /* log2(number of shards).  Shard s owns global positions whose top
                            shard_bits bits equal s; 0 = single GPU.  Any k (1..128);
                            for k > 32 a shard holds at least one tile of slots */
  uint32_t shard_id;     /* which shard this table is */
  uint64_t matrix_seed;  /* seed of the random GF(2) hash matrix; 0 = engine default.
                            All shards of one job must use the same seed */
  const uint64_t* matrix_columns; /* optional explicit matrix: 2k columns in file-header order
                            (file_header.hpp:35-64), r = log2(global size) rows; its low r x r
                            block must be invertible.  NULL = random from matrix_seed */
  uint32_t out_counter_len; /* bytes per count in dumps (binary_dumper ctor val_len,
                            count_main_cmdline.yaggo --out-counter-len); 0 = 4 */
  uint32_t matrix_kind;  /* which family the matrix comes from when neither matrix_columns nor matrix_seed is given:
                            JFGPU_MATRIX_DEFAULT (0, what the JFGPU_MATRIX environment switch says, else the reference's),
                            JFGPU_MATRIX_XORSHIFT or JFGPU_MATRIX_REFERENCE.  (Was `reserved`, always 0.) */
} jfgpu_params;

/* Matrix families.  The file format admits any r x 2k matrix with an invertible low r x r block -- readers take the
 * columns from the header (include/jellyfish/file_header.hpp:35-64) and multiply
 * (rectangular_binary_matrix.hpp:155-164) -- so the choice changes where a k-mer lands, never what is counted.
 *   REFERENCE: the matrix `jellyfish count` itself draws (lib/rectangular_binary_matrix.cc:160-247 on glibc's unseeded
 *              random()): file bodies byte-identical to the reference's, files mergeable with the reference's.
 *   XORSHIFT:  a fixed matrix per (size, k) made of xor-shift steps (jellyfish_amd/csrc/kmer_core.hpp: xs_hash), which
 *              the partition kernel evaluates in registers instead of six LDS table reads per k-mer.  One-word keys
 *              (k <= 32); longer keys get the reference family. */
enum { JFGPU_MATRIX_DEFAULT = 0, JFGPU_MATRIX_XORSHIFT = 1, JFGPU_MATRIX_REFERENCE = 2 };

/* Geometry + matrix actually used, for file_header::update_from_ary (file_header.hpp:25-33). */
typedef struct jfgpu_info {
  uint32_t k, key_len;       /* key_len = 2k */
  uint32_t canonical;
  uint32_t lsize;            /* log2(global size) = rows of the matrix */
  uint64_t size;             /* global number of slots (power of two) -> header "size" */
  uint64_t local_size;       /* slots held by this shard */
  uint32_t shard_bits, shard_id;
  uint32_t val_len;          /* bits of the in-slot count field -> header "val_len" */
  uint32_t slot_bytes;       /* 4 or 8 (one-word keys), 16 (two words), 32 (three and four) */
  uint32_t tile_slots;       /* probe domain (slots) */
  uint32_t matrix_identity;  /* 1 when size == 4^k (large_hash_array.hpp:997-1000) */
  uint32_t out_counter_len;
  uint32_t max_reprobe;      /* informational header fields (merge_files.cc:128,145-146) */
  uint64_t table_bytes;
} jfgpu_info;

typedef struct jfgpu_stats {
  uint64_t unique;     /* k-mers with count 1            (stats_main.cc:41) */
  uint64_t distinct;   /* number of different k-mers     (:44) */
  uint64_t total;      /* sum of counts                  (:42) */
  uint64_t max_count;  /*                                (:43) */
  uint64_t occupied;   /* slots in use (== distinct) */
  uint64_t mers_fed;   /* k-mer occurrences accepted by jfgpu_count_* so far */
} jfgpu_stats;

const char* jfgpu_last_error(void);       /* thread-local message of the last failing call */
int  jfgpu_abi_version(void);
int  jfgpu_device_count(void);            /* usable HIP devices (0 => nothing will work) */

/* hash_counter ctor / dtor (hash_counter.hpp:56-68). */
int  jfgpu_create(const jfgpu_params* params, jfgpu_table** out);
void jfgpu_destroy(jfgpu_table* t);
int  jfgpu_get_info(const jfgpu_table* t, jfgpu_info* out);
/* matrix() (large_hash_array.hpp:211): 2k columns, file-header order. */
int  jfgpu_get_matrix(const jfgpu_table* t, uint64_t* columns /* [2k] */);
/* array::clear() (large_hash_array.hpp:224-226). */
int  jfgpu_clear(jfgpu_table* t);
/* Block until everything enqueued so far has retired; reports a deferred
 * "Hash full" (the device cannot throw mid-kernel). == every thread called
 * hash_counter::done() (hash_counter.hpp:169-172). */
int  jfgpu_sync(jfgpu_table* t);
/* Wait until the kernels enqueued so far have finished WITHOUT applying pending partitioned
 * batches: after it returns, device buffers handed to jfgpu_count_ascii_dev / jfgpu_add_keys_dev
 * may be reused (their k-mers have been copied into the engine's workspace). */
int  jfgpu_wait(jfgpu_table* t);

/* ---- the hot path ------------------------------------------------------ */
/* mer_counter_base::start COUNT loop (sub_commands/count_main.cc:152-163) over one
 * parser-contract buffer (mer_overlap_sequence_parser.hpp:161-185: sequence
 * characters, any byte outside [ACGTacgt] resets the window, k-mers do not span
 * calls): encode (mer_iterator.hpp:53-81) -> canonical (:51) -> hash
 * (rectangular_binary_matrix.hpp:155-164) -> insert/increment
 * (large_hash_array.hpp:291-295,509-597,741-752).  Asynchronous. */
int  jfgpu_count_ascii_dev(jfgpu_table* t, const char* d_bases, size_t n);
int  jfgpu_count_ascii(jfgpu_table* t, const char* bases, size_t n);      /* host buffer (staged H2D) */

/* hash_counter::add(key, val) for a batch of already-encoded k-mers
 * (hash_counter.hpp:122-126; SWIG HashCounter.add swig/hash_counter.i:13-27).
 * is_new (optional, n bytes) receives 1 where the key was not present. */
int  jfgpu_add_keys_dev(jfgpu_table* t, const uint64_t* d_keys, size_t n, uint64_t val, uint8_t* d_is_new);
int  jfgpu_add_keys(jfgpu_table* t, const uint64_t* keys, size_t n, uint64_t val, uint8_t* is_new);

/* The same with a value per key: hash_counter::add(const mer_dna&, uint64_t val) over a batch (hash_counter.hpp:122-126 ->
 * large_hash_array.hpp:741-752 add_val) -- what loads the records of a binary/sorted file back into a table, so that
 * `query -s` (sub_commands/query_main.cc:44-51) answers from the device.  Host arrays; keys of every width (k <= 128),
 * key_words = ceil(2k / 64) words each. */
int  jfgpu_add_key_vals(jfgpu_table* t, const uint64_t* keys, const uint64_t* vals, size_t n);

/* array::get_val_for_key (large_hash_array.hpp:354-372) for a batch.  vals[i] = 0 and
 * found[i] = 0 when absent.  Keys must already be canonical if the table is. */
int  jfgpu_lookup_dev(jfgpu_table* t, const uint64_t* d_keys, size_t n, uint64_t* d_vals, uint8_t* d_found);
int  jfgpu_lookup(jfgpu_table* t, const uint64_t* keys, size_t n, uint64_t* vals, uint8_t* found);

/* query_from_sequence (sub_commands/query_main.cc:44-51; examples/query_per_sequence/query_per_sequence.cc) over one
 * parser-contract buffer, the contract of jfgpu_count_ascii_dev: mer_iterator (mer_iterator.hpp:53-81) -> canonical (:51)
 * -> array::get_val_for_key (large_hash_array.hpp:354-372) for every k-mer of the buffer, in one kernel and for every mer
 * length.  The table is only read; pending partitioned counts are applied first.  An attached Bloom counter is not asked.
 * Both outputs have n entries, indexed by the position of the k-mer's LAST base (its first base is k - 1 before):
 *   vals[p]   the k-mer's count; 0 where no k-mer ends at p or the k-mer is absent
 *   flags[p]  (optional) JFGPU_Q_MER: a k-mer ends at p; JFGPU_Q_FOUND: it is in the table; JFGPU_Q_REVCOMP: the table is
 *             canonical and the key looked up is the reverse complement of the text (never set for a palindrome)
 * Every entry is written (no memset needed), nothing beyond n.  Not for a shard (JFGPU_E_UNSUPPORTED: the keys of the
 * other shards are not here).  The _dev form is asynchronous on the table's stream; the host form stages the buffer in
 * pieces that overlap by k - 1 bytes and reports every position once. */
#define JFGPU_Q_MER     1
#define JFGPU_Q_FOUND   2
#define JFGPU_Q_REVCOMP 4
int  jfgpu_query_ascii_dev(jfgpu_table* t, const char* d_bases, size_t n, uint64_t* d_vals, uint8_t* d_flags);
int  jfgpu_query_ascii(jfgpu_table* t, const char* bases, size_t n, uint64_t* vals, uint8_t* flags);

/* ---- multi-GPU: hash-prefix partition --------------------- */
/* Encode + canonicalise + hash one contract buffer and bucket the k-mers by owning
 * shard instead of inserting them, for every mer length.  A key is key_words =
 * ceil(2k / 64) little-endian 64-bit words, the layout jfgpu_add_keys takes;
 * d_keys_out has room for `capacity` keys (capacity * key_words words).  Shard s's
 * keys are written contiguously from key offsets[s] on, in arbitrary order, with
 * counts[s] of them; offsets are the exclusive prefix sum of counts (so the buffer is
 * densely packed and ready for an all-to-all-v); capacity, counts and offsets are in
 * k-mers.  A Bloom counter attached to the table (count --bc) is asked first: what it
 * does not admit is neither counted nor written.  A one-pass filter (count --bf-size)
 * changes as it is asked and the two passes ask twice: JFGPU_E_UNSUPPORTED.
 * counts_out: host array [1 << shard_bits].  Synchronous. */
int  jfgpu_partition_ascii_dev(jfgpu_table* t, const char* d_bases, size_t n,
                               uint64_t* d_keys_out, size_t capacity, uint64_t* counts_out);

/* The exchange itself: one process per GPU, shard r = the table positions whose top shard_bits bits are
 * r.  jfgpu_comm_count_ascii_dev is one step of a rank: route this rank's contract buffer by owner, exchange (RCCL
 * ncclSend / ncclRecv over xGMI, one group per round of at most 1 GiB per peer), insert what arrived -- pipelined by
 * one step, so the keys of step i travel while step i+1 is routed and step i-1 is inserted.  Collective: every rank
 * calls it the same number of times (n may be 0), then jfgpu_comm_finish, then reads its table (jfgpu_sync, dump...);
 * the shards' sorted dumps concatenated in rank order are the globally (pos, key)-sorted file body.
 *   id128: from jfgpu_comm_unique_id on one rank, handed to the others by whatever launched them.
 * jfgpu_comm_create_local: the same code with all `world` shards in ONE process on one device and device copies as
 * the transport (no RCCL): exists so that the sharded path can be tested on a single GPU. */
typedef struct jfgpu_comm jfgpu_comm;
int  jfgpu_comm_unique_id(uint8_t* id128);
int  jfgpu_comm_create(int world, int rank, const uint8_t* id128, int device, jfgpu_comm** out);
int  jfgpu_comm_create_local(int world, int device, jfgpu_comm** out);
void jfgpu_comm_destroy(jfgpu_comm* c);
int  jfgpu_comm_count_ascii_dev(jfgpu_comm* c, jfgpu_table* t, const char* d_bases, size_t n);
int  jfgpu_comm_local_step(jfgpu_comm* c, jfgpu_table** tables, const char* const* d_bases, const size_t* n);
int  jfgpu_comm_finish(jfgpu_comm* c, uint64_t* sent, uint64_t* received);
/* What a launcher has to agree on around the steps (RCCL transport, synchronous, collective): values[n] (n <= 64) replaced
 * by their sum (op 0) or maximum (op 1) over the ranks -- "does any rank still have input?", so that every rank makes the
 * same number of steps; all[world] = every rank's `mine` -- the records each shard will write, i.e. a rank's offset in
 * the common binary/sorted file (sorted_dumper.hpp:57-101 writes one file; here shard dumps are concatenated in rank order). */
int  jfgpu_comm_allreduce_u64(jfgpu_comm* c, uint64_t* values, int n, int op);
int  jfgpu_comm_allgather_u64(jfgpu_comm* c, uint64_t mine, uint64_t* all);
int  jfgpu_comm_world(const jfgpu_comm* c, int* world, int* rank);
/* Exchange timing (measurement helper): device time of every exchange since the communicator was created or this was last
 * called -- from the moment the routed data of a step was ready on the exchange stream to the moment everything of that
 * step had been sent and received -- and the bytes this rank put on the wires for it (its own share does not travel).
 * Waits for the exchange stream.  *n = exchanges recorded; at most cap entries are written; the log is cleared. */
int  jfgpu_comm_exchange_times(jfgpu_comm* c, double* ms, uint64_t* wire_bytes, size_t cap, size_t* n);

/* ---- results path ------------------------------------------------------ */
int  jfgpu_stats_compute(jfgpu_table* t, uint64_t lower, uint64_t upper, jfgpu_stats* out);
/* Order-independent checksum of the {k-mer -> count} content restricted to lower <= count <= upper:
 * out4 = { records, sum of counts, sum of h, xor of h } (mod 2^64) with h = mix(..mix(mix(S ^ w0) ^ w1).. ^ count),
 * mix = the splitmix64 finaliser, S = 0x9E3779B97F4A7C15, w = the key's little-endian words (mer_dna::data()).
 * No reference counterpart: it exists so that a 10 Gbp run is compared with the reference's table (the oracle driver
 * computes the same numbers from large_hash_array's iterators) without writing and sorting ~86 GB of records. */
int  jfgpu_digest(jfgpu_table* t, uint64_t lower, uint64_t upper, uint64_t* out4);
/* histo_main.cc:34-45: histo[0] counts vals < base, histo[n-1] vals > ceil,
 * else histo[(val-base)/inc]. */
int  jfgpu_histo(jfgpu_table* t, uint64_t base, uint64_t ceil, uint64_t inc, uint64_t* histo, uint64_t nb_buckets);
/* sorted_dumper + binary_writer (sorted_dumper.hpp:57-101, binary_dumper.hpp:36-40):
 * produce this shard's records in ascending (pos, key) order, fixed width
 * ceil(2k/8) key bytes + out_counter_len count bytes (saturated), filtered to
 * lower <= count <= upper.  _begin returns the total record count; _next streams
 * the records in order into a host buffer of `capacity_records` records (at least
 * one tile = jfgpu_info.tile_slots), *n_read == 0 marks the end; whole tiles are
 * sorted on the device, so every chunk is a contiguous piece of the file body. */
int  jfgpu_dump_begin(jfgpu_table* t, uint64_t lower, uint64_t upper, uint64_t* n_records, uint32_t* record_bytes);
int  jfgpu_dump_next(jfgpu_table* t, void* out, uint64_t capacity_records, uint64_t* n_read);
int  jfgpu_dump_end(jfgpu_table* t);

/* ---- Bloom counter: `jellyfish bc` and `count --bc` (BASELINE config 3) -------------------
 * Mer lengths 1 to 128, like the reference's mer_dna_bloom_counter (two 64 x 2k matrices over mer_dna): every entry point
 * below -- jfgpu_bc_create, jfgpu_bf_create, the inserts, jfgpu_bc_keys, jfgpu_attach_bloom -- takes them all on one GPU.
 * Both insert strategies (jfgpu_bc_set_mode) exist for every mer length: above 32 bases (keys of two, three and four words) the
 * partitioned one routes its cell updates with a kernel of its own and shares everything behind it with the shorter mers.
 * Above 64 bases a table with a filter attached is refused by the routing and sharded entry points
 * (jfgpu_partition_ascii_dev, the jfgpu_comm_* steps) with JFGPU_E_UNSUPPORTED. */
typedef struct jfgpu_bloom jfgpu_bloom;   /* opaque: ceil(m/5) bytes of base-3 cells in HBM */
typedef struct jfgpu_bloom_params {
  uint32_t k, canonical;
  uint64_t m;                 /* number of cells (bloom_base::m(); header "size") */
  uint32_t nb_hashes;         /* header "nb_hashes" */
  int32_t  device;            /* -1 = current */
  uint64_t seed;              /* for the two random 64 x 2k matrices; 0 = default */
  const uint64_t* matrix1;    /* optional explicit matrices, 2k columns each, file-header order */
  const uint64_t* matrix2;    /*   (what load_bloom_filter reads back, count_main.cc:191-206) */
} jfgpu_bloom_params;
/* bloom_base::opt_m / opt_k (bloom_common.hpp:61-66) */
uint64_t jfgpu_bc_opt_m(double fp, uint64_t n);
uint32_t jfgpu_bc_opt_k(double fp);
/* mer_dna_bloom_counter ctor (bc_main.cc:114-120) / dtor */
int  jfgpu_bc_create(const jfgpu_bloom_params* p, jfgpu_bloom** out);
void jfgpu_bc_destroy(jfgpu_bloom* b);
/* mer_bloom_counter::start (bc_main.cc:67-71): filter.insert(*mers) for every k-mer of a contract buffer */
int  jfgpu_bc_insert_ascii_dev(jfgpu_bloom* b, const char* d_bases, size_t n);
int  jfgpu_bc_insert_ascii(jfgpu_bloom* b, const char* bases, size_t n);
int  jfgpu_bc_sync(jfgpu_bloom* b, uint64_t* mers_fed);
int  jfgpu_bc_clear(jfgpu_bloom* b);      /* all cells back to 0 (a fresh mer_dna_bloom_counter), k-mer tally reset */
int  jfgpu_bc_get_info(const jfgpu_bloom* b, uint64_t* m, uint32_t* nb_hashes, uint64_t* nb_bytes,
                       uint64_t* matrix1 /* [2k] or NULL */, uint64_t* matrix2);
/* write_bits / the istream ctor: the raw ceil(m/5) bytes of a "bloomcounter" file body */
int  jfgpu_bc_read(jfgpu_bloom* b, uint8_t* out);
int  jfgpu_bc_load(jfgpu_bloom* b, const uint8_t* data);
/* bloom_base::check / insert on encoded k-mers (query_main.cc Bloom branch); out[i] = 0, 1 or 2 (insert: the minimum before
 * it).  keys: ceil(2k / 64) little-endian words per k-mer, mer_dna::data()'s layout, key after key -- one word for
 * k <= 32, two for k <= 64, three for k <= 96, four for k <= 128; bits beyond 2k are ignored. */
int  jfgpu_bc_keys(jfgpu_bloom* b, const uint64_t* keys, size_t n, uint8_t* out, int do_insert);
/* query_from_sequence (sub_commands/query_main.cc:44-51) when the database is a Bloom counter (:99-104): check() of every
 * k-mer of one parser-contract buffer, in one kernel and for every mer length.  The contract is jfgpu_query_ascii(_dev)'s:
 * both outputs have n entries indexed by the position of the k-mer's LAST base, every entry is written and nothing beyond
 * n, flags is optional.
 *   vals[p]   check() of the k-mer (of its canonical form when the counter is canonical): 0, 1 or 2; 0 where no k-mer ends
 *   flags[p]  JFGPU_Q_MER: a k-mer ends at p; JFGPU_Q_FOUND: vals[p] != 0; JFGPU_Q_REVCOMP: the counter is canonical and the key
 *             asked is the reverse complement of the text (never set for a palindrome)
 * The counter is only read and its k-mer tally (jfgpu_bc_sync) stays; pending partitioned increments are applied first, as
 * by jfgpu_bc_keys.  A one-pass filter (jfgpu_bf_create) holds no counts: JFGPU_E_UNSUPPORTED.  The _dev form is asynchronous
 * on the counter's stream; the host form stages the buffer in pieces that overlap by k - 1 bytes and reports every
 * position once. */
int  jfgpu_bc_query_ascii_dev(jfgpu_bloom* b, const char* d_bases, size_t n, uint64_t* d_vals, uint8_t* d_flags);
int  jfgpu_bc_query_ascii(jfgpu_bloom* b, const char* bases, size_t n, uint64_t* vals, uint8_t* flags);
/* count --bf-size N --bf-fp F (count_main.cc:121-131,321-323; bloom_filter.hpp:44-68): a Bloom filter of m = opt_m(F, N)
 * BITS with opt_k(F) hashes, filled by the count itself -- attached with jfgpu_attach_bloom, every k-mer sets its bits
 * and is counted only if all of them were set before (its first sighting only marks it).  Same params struct; the
 * result is order dependent in the reference too (tests/bloom_filter.sh bounds it statistically). */
int  jfgpu_bf_create(const jfgpu_bloom_params* p, jfgpu_bloom** out);
/* How jfgpu_bc_insert_* applies the increments (no reference counterpart; the array is the same either way because the
 * increments saturate and commute): 0 auto, 1 direct (one global compare-and-swap per cell), 2 partitioned (cell updates
 * routed to 64 KiB segments of the array and applied in LDS at the next jfgpu_bc_sync / _read / _load / _keys /
 * _query_ascii / attach).  Mode 2 is accepted for every mer length up to 128 whenever the counter has a segment geometry (a
 * Bloom counter of at most 128 GiB; a one-pass filter of jfgpu_bf_create has none: JFGPU_E_UNSUPPORTED).  Auto: mers of up
 * to 32 bases take the partitioned path for batches of 1 MiB and more on counters of 64 segments and more, or while batches
 * are pending; mers of 33 to 128 bases for batches of 1 MiB and more (profiles/bloom_keys_part_rate.txt: 3.7 and 5.6 times the
 * direct kernel's rate on 2 Gbp of reads at k = 63 and k = 100); everything else goes direct.
 * jfgpu_bc_reserve sizes the routing workspace up front (default: taken from free memory at the first large batch). */
int  jfgpu_bc_set_mode(jfgpu_bloom* b, int mode);
int  jfgpu_bc_reserve(jfgpu_bloom* b, uint64_t workspace_bytes);
/* per-stage device time on the counter's stream (bench.py): which = 0 direct, 1 route (P1), 2 partition (P2), 3 segments;
 * 4: launches (no time) of the ring kernel inside stage 2, so that a test can tell which P2 kernel a flush took */
int  jfgpu_bc_profile_enable(jfgpu_bloom* b, int on);
int  jfgpu_bc_profile_get(jfgpu_bloom* b, int which, double* ms, uint64_t* launches, uint64_t* units);
int  jfgpu_bc_profile_reset(jfgpu_bloom* b);
/* count --bc: from now on jfgpu_count_* admits a k-mer only if check(m) > 1 (count_main.cc:115-118).
 * b == NULL detaches.  The Bloom counter must outlive its use.  Any mer length up to 128 (the counter's must be the
 * table's); the attachment stays when the table doubles. */
int  jfgpu_attach_bloom(jfgpu_table* t, jfgpu_bloom* b);
/* `jellyfish bc` with the input split between the GPUs (sub_commands/bc_main.cc:84-161, mer_bloom_counter::start :67-71 per
 * rank): every rank creates the same counter (jfgpu_bc_create with the same parameters: same size, same matrices), inserts
 * ITS part of the input, and calls this -- collective.  On return every rank's counter is the counter of the whole input,
 * byte for byte what one counter fed with everything holds (cells saturate at 2 and increments commute,
 * bloom_counter2.hpp:56-107): rank 0 writes the file, `count --bc --gpus` asks it on every rank.  jfgpu_bc_sync then
 * reports the k-mers of all ranks.  _local: the counters of all ranks of a local communicator, in rank order. */
int  jfgpu_comm_bc_merge(jfgpu_comm* c, jfgpu_bloom* b);
int  jfgpu_comm_bc_merge_local(jfgpu_comm* c, jfgpu_bloom** blooms);

/* hash_counter::do_size_doubling(bool) (hash_counter.hpp:78-79).  On (default): the size given at
 * creation is a hint, the table doubles itself (device-side rehash, one more matrix row) before it
 * could exceed 80 % load, as long as device memory allows; jfgpu_get_info / jfgpu_get_matrix report
 * the current geometry.  Off: a full table is the deferred error "Hash full".  The shards of a multi-GPU
 * table grow TOGETHER, inside jfgpu_comm_count_ascii_dev (abi_comm.inl: comm_grow -- every rank draws the next
 * matrix of the same stream, re-shards its entries on the device and the (key, count) pairs travel to their new
 * owners), for keys of one and two words; a shard fed outside a communicator reports "Hash full". */
int  jfgpu_set_growth(jfgpu_table* t, int on);

/* The matrix a table gets when jfgpu_params gives neither matrix_columns nor matrix_seed: the one the
 * reference itself would draw for a table of 2^lsize positions and key_len = 2k bits as the first matrix of
 * its process (RectangularBinaryMatrix::randomize_pseudo_inverse over unseeded glibc random(),
 * lib/rectangular_binary_matrix.cc:240-247, lib/misc.cc:66-72; identity when lsize >= key_len,
 * large_hash_array.hpp:997-1000).  Host only: needs no device.  columns: key_len words, file-header order. */
int  jfgpu_reference_matrix(uint32_t lsize, uint32_t key_len, uint64_t* columns);

/* What jfgpu_count_ascii(_dev) does with every k-mer (mer_counter_base::start, count_main.cc:152-184):
 *   JFGPU_OP_COUNT   add(m, 1)                                   the default
 *   JFGPU_OP_PRIME   set(m): the key enters the table with count 0   first pass of `count --if` (:289-295)
 *   JFGPU_OP_UPDATE  update_add(m, 1): counted only if already there  second pass of `count --if`
 * Keys with count 0 are real entries: stats, histo and dumps report them like the reference does. */
#define JFGPU_OP_COUNT  0
#define JFGPU_OP_PRIME  1
#define JFGPU_OP_UPDATE 2
int  jfgpu_set_operation(jfgpu_table* t, int op);

/* Device memory a table created with (k, size) occupies, and the number of positions it really gets (the size is
 * rounded up to a power of two and to the engine's minimum for that k; large_hash::array::usage_info::mem,
 * sub_commands/mem_main.cc).  Host only.  The partitioned insert path additionally needs its workspace
 * (jfgpu_reserve: about 8 bytes per k-mer fed between two syncs). */
int  jfgpu_table_bytes(uint32_t k, uint64_t size, uint64_t* slots, uint64_t* bytes);

/* Spill instead of "Hash full" when the table may not double (jfgpu_set_growth(t, 0), i.e. `count --disk`):
 * before the table would pass 80 % load the engine applies everything pending and calls fn(user); the callback
 * writes the table out as one sorted run (jfgpu_dump_begin / _next / _end -- what the reference's dumper does
 * from hash_counter::handle_full_ary, hash_counter.hpp:178-198) and returns 0; the engine then empties the table
 * and carries on.  The runs are merged afterwards (jellyfish/merge_files.cc).  fn == NULL: no spilling. */
int  jfgpu_set_spill(jfgpu_table* t, int (*fn)(void* user), void* user);

/* Insert strategy.  0 auto (default), 1 direct (global 64-bit atomics, kernels.hip.hpp),
 * 2 partitioned (radix partition + LDS-resident tiles, kernels_part.hip.hpp; large batches
 * are buffered on the device and applied at the next jfgpu_sync / read).  Results are
 * bit-identical; the environment variable JFGPU_MODE=direct|partitioned (or 1|2) sets the default.
 * Every key width has the partitioned path: one word, two words (kernels_wide_part.hip.hpp) and three and four words
 * (65 <= k <= 128, kernels_nword_part.hip.hpp, tables of up to 2^32 slots).  For keys of three and four words auto takes
 * it only where it was measured faster than the direct kernel (device batches of 1 GiB and more, k <= 100, at most 2^30
 * slots: profiles/nword_part_rate.txt), and in either mode the direct kernel
 * still inserts while a Bloom counter or one-pass filter is attached, on a shard, and for the PRIME / UPDATE operations.
 * Mode 2 is refused (JFGPU_E_UNSUPPORTED) for a geometry without the path: tiny one- and two-word tables, keys of three and
 * four words in more than 2^32 slots. */
int  jfgpu_set_mode(jfgpu_table* t, int mode);
/* Optional: pre-size the partitioned path's device workspace for `input_bytes` of sequence
 * between two syncs (what `-s` is to the table, hash_counter.hpp:56-64: a hint that moves
 * allocation out of the counting phase).  Without it the workspace grows on demand. */
int  jfgpu_reserve(jfgpu_table* t, uint64_t input_bytes);

/* ---- sequence files parsed on the device -------------------
 * Replaces mer_overlap_sequence_parser::read_fasta / read_fastq
 * (include/jellyfish/mer_overlap_sequence_parser.hpp:160-215): raw FASTA / FASTQ bytes in, the
 * contract buffer (sequence lines concatenated, headers and qualities dropped, one 'N' per record
 * boundary) out -- in device memory, ready for jfgpu_count_ascii_dev / jfgpu_bc_insert_ascii_dev /
 * jfgpu_partition_ascii_dev.
 *
 * A chunk is n <= 2^31 bytes that start at the beginning of a line and end at the end of one.
 *   FASTA  may be cut at ANY line boundary: pass JFGPU_PARSE_CONTINUE for every chunk of a file but
 *          the first and the parser prepends the previous chunk's last k-1 characters (the
 *          reference's "seam", :164-167,182-184), so no k-mer is lost or seen twice.
 *   FASTQ  chunks hold whole 4-line records.  Wrapped sequence / quality lines, blank lines or a
 *          quality string of the wrong length give JFGPU_E_FORMAT and produce nothing: pass that
 *          chunk to the host parser, which implements the reference's general reader and its
 *          "Invalid fastq sequence" error (:292-309).
 * Line ends: '\n', or any run of '\r' followed by '\n'.  A run of '\r' of ANY length is dropped where it touches a
 * '\n' or the chunk's boundary on either side (before a line's '\n', between a '\n' and the next line or its '>', at
 * the start or the end of the chunk) and kept where it stands between two other bytes of a line, as the reference's
 * unbounded loops do (:267-287); there is no run length at which this changes and none that gives JFGPU_E_FORMAT.
 * A FASTQ chunk with more than n / 8 + 16 line ends is also given JFGPU_E_FORMAT (the host parser's); at or below that
 * the device parses it.
 * The returned buffer belongs to the parser and stays valid until the second-next parse call
 * (two buffers alternate), so one chunk can be counted while the next is parsed; a call that fails
 * takes no turn and leaves the buffer of the call before it intact.  Calls are synchronous: on return
 * the buffer is complete. */
typedef struct jfgpu_parser jfgpu_parser;
#define JFGPU_PARSE_FASTA    1u
#define JFGPU_PARSE_FASTQ    2u
#define JFGPU_PARSE_CONTINUE 4u
int  jfgpu_parser_create(int device, uint32_t k, jfgpu_parser** out);
void jfgpu_parser_destroy(jfgpu_parser* p);
/* d_bytes: device memory at any alignment, readable up to the next multiple of 16 bytes.  The bytes are only read --
 * unless a minimum quality is set (jfgpu_parser_set_min_quality): then a FASTQ chunk is EDITED IN PLACE, the masked
 * bases of the caller's device buffer are 'N' on return.  jfgpu_parser_parse works on its own copy and never changes
 * the caller's host bytes. */
int  jfgpu_parser_parse_dev(jfgpu_parser* p, const char* d_bytes, size_t n, unsigned flags,
                            const char** d_out, size_t* n_out, uint64_t* n_records);
/* bytes: host memory (e.g. the mmap of the file); copied to the device, then as above. */
int  jfgpu_parser_parse(jfgpu_parser* p, const char* bytes, size_t n, unsigned flags,
                        const char** d_out, size_t* n_out, uint64_t* n_records);
/* Pinned host staging owned by the parser (which = 0 or 1, grown on demand): fill one while the other
 * is being parsed, then pass it to jfgpu_parser_parse -- the host-to-device copy of a pinned buffer runs
 * at PCIe speed, that of pageable memory (an mmap'ed file) at a fraction of it. */
int  jfgpu_parser_host_buffer(jfgpu_parser* p, int which, size_t bytes, char** out);
/* Milliseconds the parse kernels of the last call took on the device (HIP events). */
/* The same in pipeline form: _upload(which) starts the copy of a (pinned) host buffer to device buffer `which` on a copy
 * stream and returns; _upload_wait(which) says when that host buffer may be refilled; _parse_uploaded(which) parses what
 * was uploaded (waiting for that copy only).  Two buffers each side: the copy of chunk i+1 overlaps parse and count of
 * chunk i while the host reads chunk i+2. */
int  jfgpu_parser_upload(jfgpu_parser* p, int which, const char* bytes, size_t n);
int  jfgpu_parser_upload_wait(jfgpu_parser* p, int which);
int  jfgpu_parser_parse_uploaded(jfgpu_parser* p, int which, unsigned flags,
                                 const char** d_out, size_t* n_out, uint64_t* n_records);
/* count -Q / --min-quality (mer_qual_iterator.hpp:75-84, count_main.cc:234-256): from now on a FASTQ base whose quality
 * character is below min_qual_char reaches the contract buffer as 'N'.  0 switches it off.  The raw chunk given to
 * jfgpu_parser_parse_dev is edited in place when this is on.  FASTA input has no qualities: unaffected, as in the reference. */
int  jfgpu_parser_set_min_quality(jfgpu_parser* p, int min_qual_char);
int  jfgpu_parser_last_ms(jfgpu_parser* p, double* ms);

/* ---- BAM / SAM input: BGZF inflated and BAM records decoded on the device ----
 * Replaces htslib's sam_open / sam_hdr_read / sam_read1 behind jellyfish::sam_wrapper
 * (include/jellyfish/sam_format.hpp) as read by mer_overlap_sequence_parser::read_sam (:220-250) and
 * whole_sequence_parser (:192-210): BGZF members in, the contract buffer (the bases of every record,
 * one 'N' after each) out, in device memory.  Every record counts, whatever its flags; bases as
 * stored (4-bit codes 1 A, 2 C, 4 G, 8 T, anything else N); with jfgpu_parser_set_min_quality a
 * base whose quality character (char)(q + '!') is below the minimum (signed compare,
 * mer_qual_iterator.hpp:76-77) becomes N -- a missing quality (0xFF) always does.
 *
 * One BGZF member: compressed deflate data at c_off (relative to the uploaded chunk), c_len bytes,
 * inflating to isize <= 65536 bytes with the given CRC32; u_off = sum of the isize of the blocks before
 * it in the same table. */
typedef struct jfgpu_bgzf_block {
  uint64_t c_off, u_off;
  uint32_t c_len, isize, crc32, reserved;
} jfgpu_bgzf_block;
/* Host only, no device: the block table of the whole BGZF members at the start of bytes[0, n) (at most cap),
 * read from each member's XLEN and 'BC' subfield and its trailer -- nothing is inflated.  *n_used = bytes of
 * those members; a member cut by the end of the window is left out.  JFGPU_E_CORRUPT: not gzip, or gzip
 * without the BGZF field (plain gzip), or a member that inflates to more than 64 KiB. */
int  jfgpu_bgzf_scan(const void* bytes, size_t n, jfgpu_bgzf_block* out, size_t cap, size_t* n_blocks, size_t* n_used);
/* Inflate the members of the chunk uploaded into buffer `which` (jfgpu_parser_upload) on the device, one
 * wavefront per member, ISIZE and CRC32 checked per member as bgzf_read does; the output is appended to
 * the parser's inflated stream, *stream_len is its new length.  A bad member: JFGPU_E_CORRUPT naming it,
 * nothing appended. */
int  jfgpu_parser_inflate_uploaded(jfgpu_parser* p, int which, const jfgpu_bgzf_block* blocks, size_t n_blocks,
                                   size_t* stream_len);
/* Copy inflated stream bytes [offset, offset + n) to host memory (the BAM header, SAM text). */
int  jfgpu_parser_stream_read(jfgpu_parser* p, size_t offset, size_t n, void* dst);
/* Drop the first n bytes of the inflated stream. */
int  jfgpu_parser_stream_consume(jfgpu_parser* p, size_t n);
/* BAM records (sam_read1 over bam1_t, sam_format.hpp:55-95): skip the first `skip` bytes of the inflated
 * stream (the rest of the header), then decode every complete record into the contract buffer (*d_out,
 * *n_out; same lifetime rule as jfgpu_parser_parse).  n_ref (the header's reference count) only sharpens
 * the search for record starts.  The incomplete last record stays in the stream (*n_left bytes) and is
 * completed by the next jfgpu_parser_inflate_uploaded: chunks may end anywhere in a record.
 * JFGPU_E_CORRUPT: a record whose lengths do not add up. */
int  jfgpu_parser_bam_decode(jfgpu_parser* p, size_t skip, int32_t n_ref, const char** d_out, size_t* n_out,
                             uint64_t* n_records, size_t* n_left);
/* bgzip-compressed FASTA / FASTQ: the inflated stream is text, and it exists only on the device, so the cut into
 * chunks is made there.  *cut = the length of the longest prefix of the stream that jfgpu_parser_parse_dev takes as a
 * chunk of fmt (JFGPU_PARSE_FASTA: up to and including the last '\n'; JFGPU_PARSE_FASTQ: up to the last line that
 * starts with '@' and whose second-next line starts with '+'), 0 when there is none: inflate more, or -- at the end
 * of the file -- parse the whole stream. */
int  jfgpu_parser_stream_cut(jfgpu_parser* p, unsigned fmt, size_t* cut);
/* jfgpu_parser_parse_dev over the first n bytes of the inflated stream (n <= 2^31; same flags, JFGPU_PARSE_CONTINUE
 * included, same lifetime of *d_out, same quality mask), which are then dropped from it; *n_left = what stays.
 * JFGPU_E_FORMAT: nothing was produced and nothing dropped -- read the bytes back (jfgpu_parser_stream_read) for the
 * host parser. */
int  jfgpu_parser_stream_parse(jfgpu_parser* p, size_t n, unsigned flags, const char** d_out, size_t* n_out,
                               uint64_t* n_records, size_t* n_left);

/* ---- merge: k-way merge of sorted databases on the device ----
 * Replaces the heap loop of merge_files (jellyfish/merge_files.cc:36-176, driven by sub_commands/merge_main.cc) for
 * binary/sorted inputs written with one hash function: every input is sorted by (pos, key), pos = (M * key) & (size - 1);
 * the output is their union in that order with equal keys combined.  The output records are byte for byte what
 * merge_files writes after its header (binary_writer::write, binary_dumper.hpp:36-40). */
typedef struct jfgpu_merge jfgpu_merge;
typedef struct jfgpu_merge_params {
  uint32_t k;                     /* mer length, 1..128: keys of (2k+7)/8 bytes (merge_files.cc:127 key_len) */
  uint32_t n_inputs;              /* 1..255; more is JFGPU_E_UNSUPPORTED (the caller merges on the host) */
  uint64_t size;                  /* the headers' "size", a power of two (merge_files.cc:129,147-148) */
  const uint64_t* matrix_columns; /* the headers' matrix: 2k columns in file-header order; NULL = the identity flag, pos = key & (size - 1) */
  const uint32_t* counter_len;    /* [n_inputs] bytes of a count in each input, 1..8 (they may differ, merge_files.cc:139) */
  uint32_t out_counter_len;       /* bytes of a count in the output: the inputs' minimum in merge_files (:139,163) */
  uint32_t op;                    /* 0 sum, 1 min, 2 max, 3 Jaccard (sub_commands/merge_main.cc; merge_files.cc:59-100) */
  uint64_t lower, upper;          /* a combined value outside [lower, upper] is dropped; tested before it is clamped to out_counter_len bytes */
  int32_t  device;                /* HIP device ordinal, -1 = current device */
  uint32_t reserved;
  uint64_t window_records;        /* records of all inputs merged in one go; 0 = the engine's default */
} jfgpu_merge_params;
/* Receives n_records output records (n_records * ((2k+7)/8 + out_counter_len) bytes), in order; the bytes are the
 * engine's until it returns.  Non-zero stops the merge. */
typedef int (*jfgpu_merge_sink)(void* user, const void* bytes, uint64_t n_records);
int  jfgpu_merge_create(const jfgpu_merge_params* p, jfgpu_merge** out);
void jfgpu_merge_destroy(jfgpu_merge* m);
/* bodies[i]: host memory (the mmap of the file past its header) holding n_records[i] records of input i.  The position
 * range is cut into windows of about window_records records; uploads, kernels and downloads of neighbouring windows
 * overlap.  JFGPU_E_FORMAT naming the input when one is not strictly increasing in (pos, key).  op 3 writes nothing
 * (sink may be NULL): see jfgpu_merge_tallies. */
int  jfgpu_merge_run(jfgpu_merge* m, const void* const* bodies, const uint64_t* n_records, jfgpu_merge_sink sink, void* user);
/* op 3, after jfgpu_merge_run: inter, winter, union, wunion as merge_files.cc:59,91-92 tallies them. */
int  jfgpu_merge_tallies(jfgpu_merge* m, uint64_t out4[4]);
/* Milliseconds of the last run: upload (staging + host-to-device copies), kernels (HIP events), download, sink. */
int  jfgpu_merge_last_ms(jfgpu_merge* m, double out4[4]);
/* The last run's windows, records read and records written. */
int  jfgpu_merge_counts(jfgpu_merge* m, uint64_t out3[3]);

/* ---- text: binary/sorted records formatted as text on the device ----
 * Replaces the record loop of dump (sub_commands/dump_main.cc:35-52) and of the text dumper (text_dumper.hpp:18-20): the
 * records whose count lies in [lower, upper], in input order, as
 *   column  KMER<separator>COUNT\n        FASTA  >COUNT\nKMER\n
 * KMER as mer_dna::to_str (bits of the top key byte above 2k are ignored), COUNT the decimal uint64.  The bytes are those
 * the host loops write. */
#define JFGPU_TEXT_COLUMN 0
#define JFGPU_TEXT_FASTA 1
typedef struct jfgpu_text jfgpu_text;
typedef struct jfgpu_text_params {
  uint32_t k;                     /* mer length, 1..128: keys of (2k+7)/8 bytes */
  uint32_t counter_len;           /* bytes of a count in the records, 1..8 */
  uint32_t layout;                /* JFGPU_TEXT_COLUMN or JFGPU_TEXT_FASTA */
  uint32_t separator;             /* ' ' or '\t' (column layout) */
  uint64_t lower, upper;          /* records whose count is outside are dropped */
  int32_t  device;                /* HIP device ordinal, -1 = current device */
  uint32_t reserved;
  uint64_t window_records;        /* records formatted in one go by jfgpu_text_run; 0 = the engine's default */
} jfgpu_text_params;
/* Receives the text of n_records kept records (n_bytes bytes, whole lines), in order; the bytes are the engine's until it
 * returns.  Non-zero stops the run. */
typedef int (*jfgpu_text_sink)(void* user, const char* text, uint64_t n_bytes, uint64_t n_records);
int  jfgpu_text_create(const jfgpu_text_params* p, jfgpu_text** out);
void jfgpu_text_destroy(jfgpu_text* x);
/* The longest line these parameters can produce: k + 2 + digits (+ 1 for FASTA), digits those of the largest count that
 * counter_len bytes hold and upper lets through. */
int  jfgpu_text_line_max(const jfgpu_text* x, uint32_t* bytes);
/* body: host memory at any alignment (the mmap of a file past its header) holding n_records records.  Windows of
 * window_records records: window i + 1 is staged and uploaded while the kernels of window i run and the text of window
 * i - 1 comes down and goes to the sink.  A window that keeps nothing does not reach the sink. */
int  jfgpu_text_run(jfgpu_text* x, const void* body, uint64_t n_records, jfgpu_text_sink sink, void* user);
/* Device to device: d_records on a 16-byte boundary and readable up to the next one behind its last record, d_text at any
 * alignment.  *n_bytes / *n_kept: the text's bytes and lines.  JFGPU_E_INVALID, with nothing written to d_text and
 * *n_bytes the bytes needed, when they exceed capacity_bytes. */
int  jfgpu_text_format_dev(jfgpu_text* x, const void* d_records, uint64_t n_records, char* d_text, uint64_t capacity_bytes,
                           uint64_t* n_bytes, uint64_t* n_kept);
/* Milliseconds of the last run: upload (staging + host-to-device copies), kernels (HIP events), download, sink. */
int  jfgpu_text_last_ms(jfgpu_text* x, double out4[4]);
/* The last run's windows, records read, records kept and bytes written. */
int  jfgpu_text_counts(jfgpu_text* x, uint64_t out4[4]);
/* jfgpu_dump_next with the formatter between the device-sorted chunk and the copy to the host: the text of as many whole
 * tiles as fit capacity_bytes at jfgpu_text_line_max bytes a record (capacity_bytes must hold one tile) goes to out (host
 * memory); *n_records, the records of the chunk, is 0 at the end.  The table's own [lower, upper] was applied by
 * jfgpu_dump_begin; x's applies to the chunk as well (leave it at [0, 2^64 - 1] to write every record).  x's k and
 * counter_len must be the table's k and out_counter_len and both must live on one device: JFGPU_E_INVALID otherwise. */
int  jfgpu_dump_next_text(jfgpu_table* t, jfgpu_text* x, char* out, uint64_t capacity_bytes, uint64_t* n_records, uint64_t* n_bytes);

/* ---- query text: the lines of `query -s` built on the device ----
 * Replaces the line loop of query_from_sequence (sub_commands/query_main.cc:44-51): for every position p of a contract
 * buffer with JFGPU_Q_MER set, in increasing p, one line
 *   KMER COUNT\n
 * KMER the k bytes ending at p in upper case (byte & 0xDF), with JFGPU_Q_REVCOMP their reverse complement -- the form that
 * was looked up, as mer_dna::to_str prints it -- and COUNT the decimal vals[p].  vals and flags are trusted to be the answer
 * of jfgpu_query_ascii(_dev) or jfgpu_bc_query_ascii(_dev) for the same buffer; a JFGPU_Q_MER at p < k - 1 makes no line. */
typedef struct jfgpu_qtext jfgpu_qtext;
typedef struct jfgpu_qtext_params {
  uint32_t k;                /* 1..128 */
  int32_t  device;           /* -1 = current */
  uint64_t piece_positions;  /* positions looked up and formatted in one go by the host forms, at least k; 0 = the engine's
                                default (JFGPU_QUERY_PIECE, else kQueryTextPiecePositions) */
} jfgpu_qtext_params;
int  jfgpu_qtext_create(const jfgpu_qtext_params* p, jfgpu_qtext** out);
void jfgpu_qtext_destroy(jfgpu_qtext* x);
/* The longest line: k + 2 + 20. */
int  jfgpu_qtext_line_max(const jfgpu_qtext* x, uint32_t* bytes);
/* Device to device, synchronous at return like jfgpu_text_format_dev.  d_bases, d_flags and d_text at any alignment, d_vals
 * on 8 bytes; nothing outside their first n entries is read, nothing outside d_text[0, *n_bytes) written.  *n_bytes /
 * *n_lines: the text's bytes and lines.  JFGPU_E_INVALID, with nothing written to d_text and *n_bytes the bytes needed, when
 * they exceed capacity_bytes. */
int  jfgpu_qtext_format_dev(jfgpu_qtext* x, const char* d_bases, size_t n, const uint64_t* d_vals, const uint8_t* d_flags,
                            char* d_text, uint64_t capacity_bytes, uint64_t* n_bytes, uint64_t* n_lines);
/* Host forms: look-up and formatting of a host buffer (any alignment), the text handed to the sink in order, whole lines.
 * Pieces of piece_positions positions that overlap by k - 1 bytes, every line once: piece i + 1 is uploaded and looked up
 * while the text of piece i comes down and goes to the sink.  A piece without a line does not reach the sink; a sink that
 * returns non-zero stops the run (JFGPU_E_INVALID).  x's k must be the table's or counter's and both must live on one
 * device: JFGPU_E_INVALID otherwise.  A table that is a shard, a one-pass filter: JFGPU_E_UNSUPPORTED. */
int  jfgpu_query_text(jfgpu_table* t, jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, void* user);
int  jfgpu_bc_query_text(jfgpu_bloom* b, jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, void* user);
/* Milliseconds of the last run: upload (staging + host-to-device copies), kernels (look-up and format, HIP events),
 * download, sink. */
int  jfgpu_qtext_last_ms(jfgpu_qtext* x, double out4[4]);
/* The last run's pieces, positions, lines and bytes. */
int  jfgpu_qtext_counts(jfgpu_qtext* x, uint64_t out4[4]);

/* ---- sorted records: `query -s` answered from a binary/sorted body as the file has it ----
 * Replaces binary_query (include/jellyfish/binary_dumper.hpp:112-213) under query_from_sequence
 * (sub_commands/query_main.cc:44-51).  The records of such a file ascend by (pos, key), pos = (M * key) & (size - 1), and the
 * positions of hashed keys are uniform, so the body is its own index: it is uploaded unchanged, one kernel cuts it into
 * 2^bucket_bits buckets by the top bits of pos, and a look-up scans the records of its key's bucket for the key.  No table
 * is built: device memory is the body's bytes and about one byte a record, whatever k is. */
typedef struct jfgpu_sorted jfgpu_sorted;
typedef struct {
  uint32_t k, canonical, counter_len;   /* counter_len 1..8: header.counter_len() */
  uint32_t matrix_rows;                 /* header.matrix().r */
  uint64_t size;                        /* header.size(); must be 1 << matrix_rows */
  const uint64_t* matrix_columns;       /* 2k columns as in jfgpu_params; NULL: identity */
  int32_t  device;                      /* -1 = current */
  uint32_t records_per_bucket;          /* 0: the default (8) */
} jfgpu_sorted_params;
/* binary_dumper.hpp:112-213 has no counterpart: what jfgpu_sorted_create will use.  bucket_bits: the smallest B with
 * n_records >> B <= records_per_bucket, at most log2(size).  device_bytes: the body, 32 zeroed bytes behind it,
 * 8 * (2^B + 1) bytes of index and the matrix's byte tables (2048 bytes a key byte; none are kept for the identity
 * matrix).  Pure: no device is needed.  JFGPU_E_UNSUPPORTED for k > 128 or counter_len > 8, JFGPU_E_INVALID for k or
 * counter_len of 0 and a size that is no power of two. */
int  jfgpu_sorted_plan(uint64_t n_records, uint64_t size, uint32_t k, uint32_t counter_len, uint32_t records_per_bucket,
                       uint32_t* bucket_bits, uint64_t* device_bytes);
/* binary_query's constructor (binary_dumper.hpp:112-145) on the device.  body: host memory at any alignment (the mmap of
 * the file past its header) holding n_records records of ceil(2k / 8) + counter_len bytes; it is read during the call
 * only.  Fails, with nothing left allocated: JFGPU_E_INVALID "records are not in strictly increasing (pos, key) order";
 * JFGPU_E_INVALID when size is not 1 << matrix_rows; JFGPU_E_ALLOC when the device cannot take device_bytes;
 * JFGPU_E_UNSUPPORTED for k > 128 or counter_len > 8.  n_records == 0 is legal: every look-up answers "not found". */
int  jfgpu_sorted_create(const jfgpu_sorted_params* p, const void* body, uint64_t n_records, jfgpu_sorted** out);
void jfgpu_sorted_destroy(jfgpu_sorted* s);
/* n_records, bucket_bits, records of the longest bucket, device bytes held, microseconds of the upload and of the index
 * kernels in jfgpu_sorted_create. */
int  jfgpu_sorted_info(const jfgpu_sorted* s, uint64_t out6[6]);
/* query_from_sequence (query_main.cc:44-51) over one contract buffer, binary_query::check (binary_dumper.hpp:191-213) per
 * k-mer: the contract of jfgpu_query_ascii_dev / jfgpu_query_ascii, asynchronous on the object's own stream in the _dev
 * form (any later call of the same object is ordered behind it). */
int  jfgpu_sorted_query_ascii_dev(jfgpu_sorted* s, const char* d_bases, size_t n, uint64_t* d_vals, uint8_t* d_flags);
int  jfgpu_sorted_query_ascii(jfgpu_sorted* s, const char* bases, size_t n, uint64_t* vals, uint8_t* flags);
/* binary_query::check (binary_dumper.hpp:191-213) for n encoded keys, the layout and masking of jfgpu_lookup; found may
 * be NULL. */
int  jfgpu_sorted_lookup(jfgpu_sorted* s, const uint64_t* keys, size_t n, uint64_t* vals, uint8_t* found);
/* query_from_sequence (query_main.cc:44-51) with the lines built on the device: jfgpu_query_text answered by the records. */
int  jfgpu_sorted_query_text(jfgpu_sorted* s, jfgpu_qtext* x, const char* bases, size_t n, jfgpu_text_sink sink, void* user);

/* ---- measurement helpers (bench.py; not part of the reference surface) -- */
/* Per-kernel HIP-event timing on the table's stream.  which: 0 count (direct), 1 add_keys,
 * 2 shard partition, 3 lookup, 4 P1 partition, 5 P2 partition, 6 tile insert, 7 items-direct.  Returns accumulated milliseconds and launches since the
 * last reset. */
int  jfgpu_profile_enable(jfgpu_table* t, int on);
int  jfgpu_profile_get(jfgpu_table* t, int which, double* ms, uint64_t* launches, uint64_t* units);
int  jfgpu_profile_reset(jfgpu_table* t);
/* The same spans one by one, in launch order, since the last reset (at most 65536 are kept): which[i] is the slot above,
 * ms[i] the span's device time.  *n = spans recorded (may exceed cap: only cap are written).  bench.py --gpus N rebuilds
 * every step's route / split / partition / insert times from it, per rank. */
int  jfgpu_profile_spans(jfgpu_table* t, int* which, double* ms, size_t cap, size_t* n);
/* The engine's event counters since the last jfgpu_clear, after waiting for the table's stream (tests assert from them
 * which code path a flush took; `jellyfish-amd count --timing` reports them).  out[0..n): 0 tile-full events ("Hash
 * full" is raised from it), 1 k-mer occurrences fed, 2 overflow side table full, 3 side-table entries, 4 k-mers sent to
 * a shard that does not own them, 5 items inserted with global atomics by the partition kernels (ring / region
 * overflow, runs of one k-mer), 6 / 7 items placed / items past rank 3 in the sampling launch of the last flush that
 * sampled (host_partition.inl), 8 flushes that ran the plain tile kernel, 9 flushes that ran the HEAVY one, 10-13 launches
 * of the second partition level by kernel (loader / storer rings, shared rings, sort-based single pass, exact count +
 * scatter), 14 / 15 launches of the first level (ring kernel / any other), 16 launches of the tile kernel's instantiation
 * for hole-free regions (the output of the loader / storer rings), 17 launches of the tile kernel of three- and four-word
 * keys (tile_insert_nword_kernel). */
#define JFGPU_N_COUNTERS 18
int  jfgpu_get_counters(jfgpu_table* t, uint64_t* out, uint32_t n);
/* Synthetic reads: n_reads records of read_len uniform iid bases, each followed by
 * one 'N' separator (the contract buffer the parser would produce for a FASTA of
 * such reads); counter-based RNG so any slice is reproducible.  d_out needs
 * n_reads * (read_len + 1) bytes.  first_read offsets the read index. */
int  jfgpu_gen_reads_dev(jfgpu_table* t, char* d_out, uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t seed);
/* Synthetic reads of the secondary distribution "G" (BASELINE.md section 3): read_len-base windows at uniform
 * positions and strands of a uniform random genome of genome_len bases (a pure function of the seed, never stored),
 * each base substituted with probability substitution_rate; same layout and slicing rules as jfgpu_gen_reads_dev.
 * High coverage means most k-mers repeat: the case where duplicates aggregate in the LDS tiles. */
int  jfgpu_gen_genome_reads_dev(jfgpu_table* t, char* d_out, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                                uint64_t genome_len, double substitution_rate, uint64_t seed);
/* Random-access roofline denominator: n independent 64-bit atomicAdds
 * at uniformly random slots of this table's own memory (table must be cleared
 * afterwards).  Returns updates per second. */
int  jfgpu_gups(jfgpu_table* t, uint64_t n_updates, int mode, double* updates_per_s);
/* Pinned host memory: buffers handed to jfgpu_dump_next / jfgpu_count_ascii / jfgpu_memcpy_* move at PCIe speed
 * when they come from here (pageable memory goes through the runtime's staging at a fraction of it). */
int  jfgpu_malloc_host(size_t bytes, void** out);
int  jfgpu_free_host(void* p);
/* Raw device memory for callers without torch. */
int  jfgpu_malloc_dev(jfgpu_table* t, size_t bytes, void** out);
int  jfgpu_free_dev(jfgpu_table* t, void* p);
int  jfgpu_memcpy_h2d(jfgpu_table* t, void* d_dst, const void* src, size_t bytes);
int  jfgpu_memcpy_d2h(jfgpu_table* t, void* dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* JFGPU_H */
