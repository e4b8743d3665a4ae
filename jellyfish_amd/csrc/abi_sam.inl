// jellyfish_amd/csrc/abi_sam.inl -- C ABI of the BGZF inflate, the BAM record decode and the inflated FASTA / FASTQ stream
// (jfgpu_bgzf_scan, jfgpu_parser_inflate_uploaded, _stream_read, _stream_consume, _bam_decode, _stream_cut, _stream_parse),
// included by jfgpu.hip after abi_parser.inl.  BgzfState, the parser's BGZF / BAM work buffers, owns them (hip_own.hpp) and
// goes with the parser.
struct BgzfState {
  DevBuf<uint8_t> d_stream[2];
  int scur = 0; size_t stream_len = 0;                     // inflated bytes not yet consumed, in d_stream[scur]
  DevBuf<jfgpu_bgzf_block> d_blocks;
  DevBuf<unsigned long long> d_err;
  DevBuf<unsigned long long> d_cut;                        // result of stream_cut_kernel
  DevBuf<BamSeg> d_seg;
  DevBuf<uint64_t> d_want, d_rec_off, d_out_off, d_rec_start, d_rec_out;
  DevBuf<BamTotals> d_tot;
};
jfgpu_parser::jfgpu_parser() = default;
jfgpu_parser::~jfgpu_parser() = default;

namespace {

int bgzf_state(jfgpu_parser* p) {
  if(p->bgzf) return JFGPU_OK;
  std::unique_ptr<BgzfState> b(new BgzfState);
  int rc;
  if((rc = b->d_err.alloc(1)) || (rc = b->d_tot.alloc(1)) || (rc = b->d_cut.alloc(1))) return rc;
  p->bgzf = std::move(b);
  return JFGPU_OK;
}

// the stream buffer `w` holds at least `need` bytes; its first `keep` bytes survive a reallocation
int stream_reserve(jfgpu_parser* p, int w, size_t keep, size_t need) { return p->bgzf->d_stream[w].reserve_keep(keep, need, p->stream); }

const char* inflate_reason(uint32_t code) {
  switch(code) {
    case INF_BAD_TYPE: return "invalid deflate block type";
    case INF_BAD_STORED: return "stored block length check failed";
    case INF_BAD_TABLE: return "invalid Huffman code lengths";
    case INF_BAD_CODE: return "invalid Huffman code";
    case INF_BAD_DIST: return "distance too far back";
    case INF_OVERFLOW: return "more output than its ISIZE";
    case INF_OVERRUN: return "deflate data runs past the block";
    case INF_BAD_ISIZE: return "less output than its ISIZE";
    case INF_BAD_CRC: return "CRC32 mismatch";
    default: return "corrupt";
  }
}

uint32_t le32(const uint8_t* q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; }

}  // namespace

extern "C" {

int jfgpu_bgzf_scan(const void* bytes, size_t n, jfgpu_bgzf_block* out, size_t cap, size_t* n_blocks, size_t* n_used) {
  if(!n_blocks || !n_used || (n && !bytes) || (cap && !out)) return fail(JFGPU_E_INVALID, "null argument");
  const uint8_t* b = (const uint8_t*)bytes;
  size_t off = 0, nb = 0; uint64_t u = 0;
  *n_blocks = 0; *n_used = 0;
  while(nb < cap && off + 12 <= n) {
    const uint8_t* h = b + off;
    if(h[0] != 0x1f || h[1] != 0x8b || h[2] != 8)
      return fail(JFGPU_E_CORRUPT, "not a gzip member at offset " + std::to_string(off));
    const uint32_t flg = h[3];
    if(!(flg & 4)) return fail(JFGPU_E_CORRUPT, "gzip member without the BGZF extra field at offset " + std::to_string(off) + " (plain gzip is not BGZF)");
    const size_t xlen = (size_t)h[10] | (size_t)h[11] << 8;
    if(off + 12 + xlen > n) break;                           // header not complete in this window
    size_t bsize = 0; bool have = false;
    for(size_t x = 12; x + 4 <= 12 + xlen;) {
      const size_t slen = (size_t)h[x + 2] | (size_t)h[x + 3] << 8;
      if(h[x] == 'B' && h[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) { bsize = (size_t)h[x + 4] | (size_t)h[x + 5] << 8; have = true; }
      x += 4 + slen;
    }
    if(!have) return fail(JFGPU_E_CORRUPT, "gzip member without the BGZF 'BC' field at offset " + std::to_string(off) + " (plain gzip is not BGZF)");
    const size_t size = bsize + 1;
    if(off + size > n) break;                                // member not complete in this window
    size_t hl = 12 + xlen;
    for(uint32_t f = 8; f <= 16; f <<= 1)                    // FNAME, FCOMMENT: zero-terminated
      if(flg & f) { while(hl < size && h[hl]) ++hl; ++hl; }
    if(flg & 2) hl += 2;                                     // FHCRC
    if(hl + 8 > size) return fail(JFGPU_E_CORRUPT, "BGZF member at offset " + std::to_string(off) + " is shorter than its header");
    jfgpu_bgzf_block& o = out[nb];
    o.c_off = off + hl; o.u_off = u; o.c_len = (uint32_t)(size - hl - 8);
    o.crc32 = le32(h + size - 8); o.isize = le32(h + size - 4); o.reserved = 0;
    if(o.isize > 65536) return fail(JFGPU_E_CORRUPT, "BGZF member at offset " + std::to_string(off) + " inflates to more than 64 KiB");
    u += o.isize; off += size; ++nb;
  }
  *n_blocks = nb; *n_used = off;
  return JFGPU_OK;
}

int jfgpu_parser_inflate_uploaded(jfgpu_parser* p, int which, const jfgpu_bgzf_block* blocks, size_t n_blocks, size_t* stream_len) {
  int rc = use_p(p); if(rc) return rc;
  if(which < 0 || which > 1 || !p->copy_stream) return fail(JFGPU_E_INVALID, "nothing was uploaded");
  if(n_blocks && !blocks) return fail(JFGPU_E_INVALID, "null block table");
  if(n_blocks > (size_t)1 << 30) return fail(JFGPU_E_INVALID, "too many blocks");
  rc = bgzf_state(p); if(rc) return rc;
  BgzfState& b = *p->bgzf;
  uint64_t total = 0;
  for(size_t i = 0; i < n_blocks; ++i) {                       // nothing the kernel reads or writes may leave its buffers
    const jfgpu_bgzf_block& k = blocks[i];
    if(k.u_off != total || k.isize > 65536 || k.c_off + (uint64_t)k.c_len + 8 > p->up_len[which])
      return fail(JFGPU_E_INVALID, "block table entry " + std::to_string(i) + " does not fit the uploaded bytes");
    total += k.isize;
  }
  const int w = b.scur;
  rc = stream_reserve(p, w, b.stream_len, b.stream_len + total + 64); if(rc) return rc;
  if(n_blocks) {
    rc = b.d_blocks.reserve(n_blocks); if(rc) return rc;
    HIP_TRY(hipStreamWaitEvent(p->stream, p->up_done[which], 0));
    HIP_TRY(hipMemcpyAsync(b.d_blocks, blocks, n_blocks * sizeof(jfgpu_bgzf_block), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemsetAsync(b.d_err, 0xFF, sizeof(unsigned long long), p->stream));
    HIP_TRY(hipEventRecord(p->ev_a, p->stream));
    rc = launch_lds(bgzf_inflate_kernel, dim3((unsigned)n_blocks), dim3(64), kInfLds, p->stream, (const uint8_t*)p->d_up[which], b.d_blocks,
                    b.d_stream[w] + b.stream_len, b.d_err);
    if(rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(p->ev_b, p->stream));
    unsigned long long err = 0;
    HIP_TRY(hipMemcpyAsync(&err, b.d_err, sizeof(err), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    if(hipEventElapsedTime(&ms, p->ev_a, p->ev_b) == hipSuccess) p->last_ms = ms;
    if(err != ~0ull) {
      const size_t blk = (size_t)(err >> 8);
      return fail(JFGPU_E_CORRUPT, "BGZF block " + std::to_string(blk) + " (deflate data at byte " + std::to_string(blocks[blk].c_off) +
                                       " of the chunk): " + inflate_reason((uint32_t)(err & 255)));
    }
  }
  b.stream_len += total;
  if(stream_len) *stream_len = b.stream_len;
  return JFGPU_OK;
}

int jfgpu_parser_stream_read(jfgpu_parser* p, size_t offset, size_t n, void* dst) {
  int rc = use_p(p); if(rc) return rc;
  const size_t have = p->bgzf ? p->bgzf->stream_len : 0;
  if(offset > have || n > have - offset) return fail(JFGPU_E_INVALID, "read past the inflated stream");
  if(n && !dst) return fail(JFGPU_E_INVALID, "null buffer");
  if(!n) return JFGPU_OK;
  HIP_TRY(hipMemcpyAsync(dst, p->bgzf->d_stream[p->bgzf->scur] + offset, n, hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return JFGPU_OK;
}

int jfgpu_parser_stream_consume(jfgpu_parser* p, size_t n) {
  int rc = use_p(p); if(rc) return rc;
  const size_t have = p->bgzf ? p->bgzf->stream_len : 0;
  if(n > have) return fail(JFGPU_E_INVALID, "consume past the inflated stream");
  if(!n) return JFGPU_OK;
  BgzfState& b = *p->bgzf;
  const size_t left = have - n;
  if(left) {                                                   // the tail moves to the front of the other buffer
    const int o = b.scur ^ 1;
    rc = stream_reserve(p, o, 0, left + 64); if(rc) return rc;
    HIP_TRY(hipMemcpyAsync(b.d_stream[o], b.d_stream[b.scur] + n, left, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    b.scur = o;
  }
  b.stream_len = left;
  return JFGPU_OK;
}

int jfgpu_parser_bam_decode(jfgpu_parser* p, size_t skip, int32_t n_ref, const char** d_out, size_t* n_out, uint64_t* n_records, size_t* n_left) {
  int rc = use_p(p); if(rc) return rc;
  if(!d_out || !n_out) return fail(JFGPU_E_INVALID, "null argument");
  *d_out = nullptr; *n_out = 0;
  if(n_records) *n_records = 0;
  if(n_ref < 0) return fail(JFGPU_E_INVALID, "negative reference count");
  rc = bgzf_state(p); if(rc) return rc;
  BgzfState& b = *p->bgzf;
  const uint64_t n = b.stream_len;
  if(skip > n) return fail(JFGPU_E_INVALID, "skip past the inflated stream");
  const uint64_t nseg64 = (n - skip + kBamSeg - 1) / kBamSeg;
  if(nseg64 > ((uint64_t)1 << 24)) return fail(JFGPU_E_INVALID, "inflated stream too large for one call");
  const uint32_t nseg = (uint32_t)nseg64;
  BamTotals tot = {0, 0, skip, 0, 0};
  if(nseg) {
    const uint8_t* S = b.d_stream[b.scur];
    if((rc = b.d_seg.reserve(nseg)) || (rc = b.d_want.reserve(nseg)) || (rc = b.d_rec_off.reserve(nseg)) || (rc = b.d_out_off.reserve(nseg))) return rc;
    HIP_TRY(hipEventRecord(p->ev_a, p->stream));
    hipLaunchKernelGGL(bam_guess_kernel, dim3((nseg + 255) / 256), dim3(256), 0, p->stream, S, n, (uint64_t)skip, nseg, n_ref, b.d_seg);
    hipLaunchKernelGGL(bam_fix_kernel, dim3(1), dim3(1024), 0, p->stream, S, n, (uint64_t)skip, nseg, b.d_seg, b.d_want, b.d_rec_off, b.d_out_off, b.d_tot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&tot, b.d_tot, sizeof(tot), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if(tot.bad) return fail(JFGPU_E_CORRUPT, "BAM record whose lengths do not add up (corrupt stream)");
    if(tot.recs) {
      const int w = p->cur; p->cur ^= 1;
      if((rc = b.d_rec_start.reserve(tot.recs)) || (rc = b.d_rec_out.reserve(tot.recs)) || (rc = p->d_out[w].reserve(tot.out + 64))) return rc;
      hipLaunchKernelGGL(bam_list_kernel, dim3((nseg + 255) / 256), dim3(256), 0, p->stream, S, n, (uint64_t)skip, nseg, b.d_seg, b.d_rec_off, b.d_out_off,
                         b.d_rec_start, b.d_rec_out);
      const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((tot.recs + 3) / 4, 16384));
      hipLaunchKernelGGL(bam_emit_kernel, dim3(grid), dim3(256), 0, p->stream, S, tot.recs, b.d_rec_start, b.d_rec_out, p->min_qual, p->d_out[w]);
      HIP_TRY(hipGetLastError());
      *d_out = (const char*)p->d_out[w].get(); *n_out = tot.out;
    }
    HIP_TRY(hipEventRecord(p->ev_b, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    float ms = 0;
    if(hipEventElapsedTime(&ms, p->ev_a, p->ev_b) == hipSuccess) p->last_ms = ms;
  }
  rc = jfgpu_parser_stream_consume(p, (size_t)tot.end); if(rc) return rc;    // the incomplete last record stays
  if(n_records) *n_records = tot.recs;
  if(n_left) *n_left = b.stream_len;
  return JFGPU_OK;
}

int jfgpu_parser_stream_cut(jfgpu_parser* p, unsigned fmt, size_t* cut) {
  int rc = use_p(p); if(rc) return rc;
  if(!cut) return fail(JFGPU_E_INVALID, "null argument");
  *cut = 0;
  if(fmt != JFGPU_PARSE_FASTA && fmt != JFGPU_PARSE_FASTQ) return fail(JFGPU_E_INVALID, "format must be JFGPU_PARSE_FASTA or JFGPU_PARSE_FASTQ");
  const size_t n = p->bgzf ? p->bgzf->stream_len : 0;
  if(!n) return JFGPU_OK;
  BgzfState& b = *p->bgzf;                                     // (the stream buffer has 64 bytes of slack behind stream_len)
  HIP_TRY(hipEventRecord(p->ev_a, p->stream));
  hipLaunchKernelGGL(stream_cut_kernel, dim3(1), dim3(kCutBlock), 0, p->stream, (const uint8_t*)b.d_stream[b.scur], (uint64_t)n,
                     fmt == JFGPU_PARSE_FASTA ? (uint32_t)PARSE_FASTA : (uint32_t)PARSE_FASTQ, b.d_cut);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(p->ev_b, p->stream));
  unsigned long long c = 0;
  HIP_TRY(hipMemcpyAsync(&c, b.d_cut, sizeof(c), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  float ms = 0;
  if(hipEventElapsedTime(&ms, p->ev_a, p->ev_b) == hipSuccess) p->last_ms = ms;
  *cut = (size_t)c;
  return JFGPU_OK;
}

int jfgpu_parser_stream_parse(jfgpu_parser* p, size_t n, unsigned flags, const char** d_out, size_t* n_out, uint64_t* n_records, size_t* n_left) {
  int rc = use_p(p); if(rc) return rc;
  if(!d_out || !n_out) return fail(JFGPU_E_INVALID, "null argument");
  *d_out = nullptr; *n_out = 0;
  if(n_records) *n_records = 0;
  const size_t have = p->bgzf ? p->bgzf->stream_len : 0;
  if(n > ((size_t)1 << 31)) return fail(JFGPU_E_INVALID, "chunk larger than 2^31 bytes");
  if(n > have) return fail(JFGPU_E_INVALID, "parse past the inflated stream");
  // (the stream buffer is an allocation's start: 16-byte aligned, as parse_dev's vector loads like it)
  rc = jfgpu_parser_parse_dev(p, n ? (const char*)p->bgzf->d_stream[p->bgzf->scur].get() : nullptr, n, flags, d_out, n_out, n_records);
  if(rc) return rc;                                            // JFGPU_E_FORMAT: nothing consumed, the bytes can be read back
  const double ms = p->last_ms;
  rc = jfgpu_parser_stream_consume(p, n); if(rc) return rc;
  p->last_ms = n ? ms : 0;
  if(n_left) *n_left = have - n;
  return JFGPU_OK;
}

}  // extern "C"
