// jellyfish_amd/include/jellyfish_amd/sam_parser.hpp
//
// `count --sam`: SAM / BAM files -> contract buffers (every record's bases, one 'N' after each), the role of
// jellyfish::sam_wrapper (include/jellyfish/sam_format.hpp) under mer_overlap_sequence_parser::read_sam (:220-250).
// The input type is sniffed from the first bytes:
//   BGZF whose stream starts "BAM\1"  the device path: the host walks the member headers (jfgpu_bgzf_scan), whole members
//                                      go to the device in chunks, are inflated there (CRC32 / ISIZE checked) and the
//                                      records decoded there (jfgpu_parser_bam_decode); the host reads only the header
//   other BGZF                        BGZF-compressed SAM text: inflated on the device, copied back, tokenised here
//   "CRAM", plain (non-BGZF) gzip     refused with a message naming the format
//   anything else                     SAM text, tokenised here (an interchange format, not the bulk path)
// Every record counts, whatever its flags; bases as stored; a record's k-mers never join the next record's.  With a
// minimum quality a base whose quality character is below it becomes 'N' (a missing quality always does).
#pragma once
#include <jfgpu.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

namespace jellyfish_amd {

class sam_parser {
public:
  typedef std::function<void(const char* d_buf, size_t n)> dev_sink_type;   // contract buffer in device memory
  typedef std::function<void(const char* buf, size_t n)> host_sink_type;    // contract buffer in host memory
  typedef std::function<void()> fence_type;                                 // "buffers handed out earlier may be reused"

  sam_parser(unsigned mer_len, int device, size_t chunk_bytes = (size_t)64 << 20) : chunk_(chunk_bytes) {
    if(const char* e = getenv("JFGPU_PARSE_CHUNK")) {          // testing / tuning knob (shared with the FASTA / FASTQ feed)
      const size_t v = strtoull(e, nullptr, 10);
      if(v) chunk_ = v;
    }
    chunk_ = std::min<size_t>(std::max<size_t>(chunk_, 1), (size_t)1 << 30);
    if(jfgpu_parser_create(device, mer_len, &p_)) throw std::runtime_error(jfgpu_last_error());
  }
  ~sam_parser() { jfgpu_parser_destroy(p_); }
  sam_parser(const sam_parser&) = delete;
  sam_parser& operator=(const sam_parser&) = delete;

  void min_quality(int c) {
    min_qual_ = c;
    if(jfgpu_parser_set_min_quality(p_, c)) throw std::runtime_error(jfgpu_last_error());
  }
  size_t nb_reads() const { return reads_; }
  // The per-chunk buffers (two pinned staging buffers, two block tables) for files of up to `largest_file` bytes,
  // allocated once: the CLI calls it in its Init phase, as the FASTA / FASTQ feed does with its staging buffers.
  void prepare(size_t largest_file) {
    const size_t w = std::min(window(), largest_file);
    if(w <= prepared_) return;
    for(int i = 0; i < 2; ++i) {
      char* pin = nullptr;
      if(jfgpu_parser_host_buffer(p_, i, w + 64, &pin)) throw std::runtime_error(jfgpu_last_error());
      blocks_[i].resize(w / 28 + 1);                           // a BGZF member is at least 28 bytes
    }
    prepared_ = w;
  }
  double device_ms() const { return device_ms_; }

  void parse_file(const char* path, const dev_sink_type& dev_sink, const host_sink_type& host_sink, const fence_type& fence) {
    path_ = path;
    int fd = open(path, O_RDONLY);
    if(fd < 0) throw std::runtime_error(std::string("Can't open SAM/BAM file '") + path + "'");
    struct stat st;
    std::vector<char> whole;                                   // pipes: read into memory
    const char* data = nullptr; size_t size = 0; void* m = MAP_FAILED;
    if(fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
      size = (size_t)st.st_size;
      if(size) {
        m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if(m == MAP_FAILED) { close(fd); throw std::runtime_error(std::string("Can't mmap '") + path + "'"); }
        madvise(m, size, MADV_SEQUENTIAL);
        data = (const char*)m;
      }
    } else {
      char buf[1 << 16]; ssize_t r;
      while((r = read(fd, buf, sizeof buf)) > 0) whole.insert(whole.end(), buf, buf + r);
      data = whole.data(); size = whole.size();
    }
    close(fd);
    try {
      const unsigned char* u = (const unsigned char*)data;
      if(size >= 4 && !memcmp(data, "CRAM", 4)) throw error("is CRAM: CRAM input is not supported (it needs the reference sequence)");
      if(size >= 2 && u[0] == 0x1f && u[1] == 0x8b) {
        // the member header scan decides (the 'BC' subfield may sit anywhere in the extra field)
        jfgpu_bgzf_block first; size_t nb = 0, u = 0;
        if(jfgpu_bgzf_scan(data, size, &first, 1, &nb, &u) == JFGPU_E_CORRUPT)
          throw error(std::string("is gzip but not BGZF (") + jfgpu_last_error() + "): plain gzip input is not supported (recompress it with bgzip)");
        parse_bgzf(data, size, dev_sink, host_sink, fence);
      } else {
        sam_text text(*this, host_sink);
        text.feed(data, size);
        text.finish();
      }
    } catch(...) { if(m != MAP_FAILED) munmap(m, size); throw; }
    if(m != MAP_FAILED) munmap(m, size);
  }

private:
  std::runtime_error error(const std::string& what) const { return std::runtime_error("SAM/BAM file '" + path_ + "' " + what); }

  // SAM text lines -> contract buffer in host memory: '@' lines are the header, column 10 SEQ, column 11 QUAL.  htslib's
  // 4-bit table maps upper- and lower-case ACGT to A C G T and everything else to N; SEQ '*' has no bases; QUAL '*' is a
  // missing quality (the quality character ' ' for every base, as a BAM 0xFF reads).
  class sam_text {
  public:
    sam_text(sam_parser& o, const host_sink_type& sink) : o_(o), sink_(sink) {}
    void feed(const char* d, size_t n) {
      size_t a = 0;
      if(!line_.empty()) {                                     // the line cut by the previous piece
        const void* q = memchr(d, '\n', n);
        const size_t e = q ? (size_t)((const char*)q - d) : n;
        line_.append(d, e);
        if(!q) return;
        take(line_.data(), line_.size());
        line_.clear();
        a = e + 1;
      }
      while(a < n) {
        const void* q = memchr(d + a, '\n', n - a);
        if(!q) { line_.assign(d + a, n - a); break; }
        const size_t e = (size_t)((const char*)q - d);
        take(d + a, e - a);
        a = e + 1;
      }
      if(out_.size() >= ((size_t)4 << 20)) flush();
    }
    void finish() {
      if(!line_.empty()) { take(line_.data(), line_.size()); line_.clear(); }
      flush();
    }
  private:
    void flush() { if(!out_.empty()) sink_(out_.data(), out_.size()); out_.clear(); }
    void take(const char* l, size_t n) {
      ++line_no_;
      if(n && l[n - 1] == '\r') --n;
      if(n == 0 || l[0] == '@') return;
      const char* f[12]; size_t fl[12]; int nf = 0;
      size_t s = 0;
      for(size_t i = 0; i <= n && nf < 12; ++i)
        if(i == n || l[i] == '\t') { f[nf] = l + s; fl[nf] = i - s; ++nf; s = i + 1; }
      if(nf < 11) throw o_.error("line " + std::to_string(line_no_) + ": fewer than 11 columns");
      const char* seq = f[9]; size_t ls = fl[9];
      const char* qual = f[10]; const size_t lq = fl[10];
      if(ls == 1 && seq[0] == '*') ls = 0;
      const bool no_qual = lq == 1 && qual[0] == '*';
      if(ls && !no_qual && lq != ls) throw o_.error("line " + std::to_string(line_no_) + ": SEQ and QUAL are of different length");
      ++o_.reads_;
      for(size_t i = 0; i < ls; ++i) {
        char c;
        switch(seq[i]) {
          case 'A': case 'a': c = 'A'; break;
          case 'C': case 'c': c = 'C'; break;
          case 'G': case 'g': c = 'G'; break;
          case 'T': case 't': c = 'T'; break;
          default: c = 'N';
        }
        // a missing quality is stored as 0xFF and read back as (char)(0xFF + '!') = ' ', as in the BAM path
        if(o_.min_qual_ && (int)(signed char)(no_qual ? ' ' : qual[i]) < o_.min_qual_) c = 'N';
        out_.push_back(c);
      }
      out_.push_back('N');
    }
    sam_parser& o_;
    const host_sink_type& sink_;
    std::string line_, out_;
    size_t line_no_ = 0;
  };

  // The header (magic, l_text, text, n_ref, references) from the first bytes of the stream: its length, or 0 when
  // more bytes are needed.
  size_t bam_header_length(const std::string& h, int32_t& n_ref) const {
    auto i32 = [&](size_t at) { int32_t v; memcpy(&v, h.data() + at, 4); return v; };
    if(h.size() < 4) return 0;
    if(memcmp(h.data(), "BAM\1", 4)) throw error("is not BAM: bad magic in the inflated stream");
    if(h.size() < 12) return 0;
    const int32_t l_text = i32(4);
    if(l_text < 0) throw error("has a corrupt BAM header (negative text length)");
    size_t at = 8 + (size_t)l_text;
    if(h.size() < at + 4) return 0;
    n_ref = i32(at);
    if(n_ref < 0) throw error("has a corrupt BAM header (negative reference count)");
    at += 4;
    for(int32_t r = 0; r < n_ref; ++r) {
      if(h.size() < at + 4) return 0;
      const int32_t l_name = i32(at);
      if(l_name < 1) throw error("has a corrupt BAM header (reference name length)");
      at += 4 + (size_t)l_name + 4;
      if(h.size() < at) return 0;
    }
    return at;
  }

  // BGZF: chunks of whole members (at most chunk_ compressed bytes, at least one member), each uploaded while the
  // previous one is decoded (two pinned buffers), inflated on the device, then decoded as BAM or copied back as SAM text.
  void parse_bgzf(const char* data, size_t size, const dev_sink_type& dev_sink, const host_sink_type& host_sink, const fence_type& fence) {
    enum { UNKNOWN, BAM_HEADER, BAM_RECORDS, SAM_TEXT } kind = UNKNOWN;
    std::string hdr;                                           // BAM header bytes read so far
    int32_t n_ref = 0;
    sam_text text(*this, host_sink);
    std::vector<jfgpu_bgzf_block>* blocks = blocks_;
    size_t used[2] = {0, 0}, nblk[2] = {0, 0};                 // bytes and members of the chunk in buffer w
    const size_t window = this->window();
    prepare(size);
    auto scan = [&](size_t pos, int w) {                       // the block table of the chunk at pos
      const size_t n = std::min(window, size - pos);
      size_t nb = 0, u = 0;
      if(jfgpu_bgzf_scan(data + pos, n, blocks[w].data(), blocks[w].size(), &nb, &u))
        throw error(std::string("is corrupt: ") + jfgpu_last_error() + " (byte " + std::to_string(pos) + " of the file)");
      if(nb == 0) throw error("is truncated: incomplete BGZF member at byte " + std::to_string(pos));
      nblk[w] = nb; used[w] = u;
    };
    auto upload = [&](size_t pos, int w) {
      char* pin = nullptr;
      if(jfgpu_parser_host_buffer(p_, w, used[w] + 64, &pin)) throw std::runtime_error(jfgpu_last_error());
      memcpy(pin, data + pos, used[w]);
      if(jfgpu_parser_upload(p_, w, pin, used[w])) throw std::runtime_error(jfgpu_last_error());
    };
    size_t pos = 0;
    scan(0, 0); upload(0, 0);
    for(int w = 0; pos < size; w ^= 1) {
      const size_t next = pos + used[w];
      if(next < size) { scan(next, w ^ 1); upload(next, w ^ 1); }   // (buffer w^1's last chunk was inflated: both sides are free)
      size_t slen = 0;
      if(jfgpu_parser_inflate_uploaded(p_, w, blocks[w].data(), nblk[w], &slen)) {
        throw error(std::string("could not be inflated: ") + jfgpu_last_error() + " (chunk at byte " + std::to_string(pos) + " of the file)");
      }
      add_ms();
      if(kind == UNKNOWN && slen >= 4) {
        char magic[4];
        read_stream(0, 4, magic);
        kind = memcmp(magic, "BAM\1", 4) ? SAM_TEXT : BAM_HEADER;
      }
      if(kind == SAM_TEXT || (kind == UNKNOWN && next >= size)) {
        std::vector<char> buf(slen);
        read_stream(0, slen, buf.data());
        consume(slen);
        text.feed(buf.data(), slen);
      } else if(kind == BAM_HEADER) {
        // read back only as much as the header needs: 64 KiB first, the rest of the chunk if that was not enough
        const size_t before = hdr.size();
        size_t got = std::min<size_t>(slen, 65536), H = 0;
        hdr.resize(before + got);
        read_stream(0, got, &hdr[before]);
        if(!(H = bam_header_length(hdr, n_ref)) && got < slen) {
          hdr.resize(before + slen);
          read_stream(got, slen - got, &hdr[before + got]);
          got = slen;
          H = bam_header_length(hdr, n_ref);
        }
        if(H) { kind = BAM_RECORDS; decode(H - before, n_ref, dev_sink, fence); hdr.clear(); }
        else consume(slen);
      } else if(kind == BAM_RECORDS) {
        decode(0, n_ref, dev_sink, fence);
      }
      pos = next;
    }
    if(kind == BAM_HEADER) throw error("is truncated: the BAM header is incomplete");
    if(kind == BAM_RECORDS && left_) throw error("is truncated: " + std::to_string(left_) + " bytes of an incomplete BAM record at the end");
    text.finish();
    left_ = 0;
  }

  void decode(size_t skip, int32_t n_ref, const dev_sink_type& dev_sink, const fence_type& fence) {
    fence();                                                   // the output buffer of two calls ago is reused
    const char* d_out = nullptr; size_t n_out = 0; uint64_t recs = 0;
    if(jfgpu_parser_bam_decode(p_, skip, n_ref, &d_out, &n_out, &recs, &left_)) throw error(std::string("is corrupt: ") + jfgpu_last_error());
    add_ms();
    reads_ += recs;
    if(n_out) dev_sink(d_out, n_out);
  }
  void read_stream(size_t off, size_t n, char* dst) { if(jfgpu_parser_stream_read(p_, off, n, dst)) throw std::runtime_error(jfgpu_last_error()); }
  void consume(size_t n) { if(jfgpu_parser_stream_consume(p_, n)) throw std::runtime_error(jfgpu_last_error()); }
  void add_ms() { double ms = 0; jfgpu_parser_last_ms(p_, &ms); device_ms_ += ms; }

  size_t window() const { return std::max<size_t>(chunk_, (size_t)65536 + 32); }   // compressed bytes per chunk, one member at least

  jfgpu_parser* p_ = nullptr;
  size_t chunk_;
  size_t prepared_ = 0;                                        // compressed bytes the chunk buffers hold
  std::vector<jfgpu_bgzf_block> blocks_[2];
  int min_qual_ = 0;
  size_t reads_ = 0, left_ = 0;
  double device_ms_ = 0;
  std::string path_;
};

}  // namespace jellyfish_amd
