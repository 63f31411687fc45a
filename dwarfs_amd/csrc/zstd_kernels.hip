// zstd_kernels.hip -- Zstandard frame decode on the GPU (gfx950) in three
// launches on the caller's stream; the kernel boundary orders them, there are
// no flags or atomics between workgroups.  The contracts and the malformed-input
// rules are stated at the top of zstd_host.cpp, which holds the sequential
// restatement; the parsers, bit readers and table builders both sides use are
// in zstd_common.h.
//
//   index    one lane per frame, one workgroup: the frame header and the block
//            headers, and of a Compressed block only its literals-section
//            header and its sequences header.  Per block a record: type, where
//            its sections start, which earlier block supplies its Huffman tree
//            (Treeless) and each Repeat table, and where its literals and
//            sequence records go in the workspace.  Slots are dealt out frame by
//            frame, to the valid frames first; one that does not fit what the
//            caller promised gets RPP_OUTPUT_TOO_SMALL and nothing of it is
//            decoded.  A frame whose walk fails at a block keeps the blocks
//            before it, so that what they produce is written as the contract
//            says, where slots are left behind the valid frames'; its status
//            stays corrupt.
//   entropy  one wave per block, kEntropyWaves per workgroup.  Entropy decoding
//            needs no output byte of an earlier block, so every block of every
//            frame runs at once.  Lane 0 builds the Huffman table (2^11 entries)
//            in LDS, the four literal streams decode in four lanes, then lane 0
//            builds the three FSE tables in LDS and decodes the sequences into
//            (literal length, match length, offset value) records.  A block that
//            uses Treeless or Repeat rebuilds the table from the supplying
//            block's description.
//   execute  one wave per frame: resolves the repeat offsets and copies literals
//            and matches with the whole wave, as rpp_lz4_decode_kernel does
//            (lz4_kernels.hip: wave_copy, the pattern copy for offset < length,
//            and the store watermark with `s_waitcnt vmcnt(0)` before a match
//            that reads bytes stored since the last wait).
//
// Every loop is bounded by a size read beforehand: it either consumes input
// bits or bytes, or produces a counted symbol.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ricepp_amd.h"
#include "zstd_common.h"

namespace {

using namespace rpp_zstd;

constexpr uint32_t kWave = 64;
constexpr uint32_t kIndexThreads = 256;
constexpr uint32_t kEntropyWaves = 4;  // blocks per entropy workgroup
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kSlack = 16;        // sequence records beyond a third of the promised bytes

struct FrameRec {
  int32_t status;
  uint32_t nblocks, block_base, block_max;
  uint64_t lit_base, seq_base, window;
};

struct BlockRec {
  uint32_t frame, kind, pos, size;  // pos: of the content in the frame
  uint32_t lit_kind, lit_hdr, lit_regen, lit_comp, lit_streams;
  uint32_t huf_src;                              // the block (of the frame) whose tree description is used
  uint32_t seq_pos, seq_count, seq_hdr, modes;   // seq_pos: of the sequences section in the frame
  uint32_t tab_src[3];                           // the block whose description of table k is used
  uint32_t lit_at, seq_at;                       // in the frame's literal bytes and sequence records
  int32_t status;                                // written by the entropy kernel
};

struct Ws {
  uint32_t* used;  // [1] block slots dealt out
  FrameRec* frames;
  BlockRec* blocks;
  Seq* seqs;
  uint8_t* lits;
  uint32_t max_blocks;
  uint64_t seq_cap, lit_cap;
};

__device__ inline uint32_t lane_id() { return threadIdx.x & (kWave - 1); }

// n bytes from s to d, the two ranges apart; 4 bytes per lane while 256 are left
__device__ inline void wave_copy(uint8_t* d, const uint8_t* s, uint64_t n, uint32_t lane) {
  uint64_t k = 0;
  for (; k + 256 <= n; k += 256) {
    uint32_t v;
    __builtin_memcpy(&v, s + k + 4 * lane, 4);
    __builtin_memcpy(d + k + 4 * lane, &v, 4);
  }
  for (uint64_t j = k + lane; j < n; j += kWave) d[j] = s[j];
}

// ---------------------------------------------------------------------------
// index
// ---------------------------------------------------------------------------
// Walks one frame; with `recs` it writes the first `cap` block records.  The frame's status; fr.nblocks counts
// the blocks walked without fault, also where a later one fails.
__device__ int32_t walk_frame(const uint8_t* in, uint64_t in_n, uint64_t out_n, uint32_t frame, FrameRec& fr,
                              BlockRec* recs, uint32_t cap) {
  if (in_n >> 32 || out_n >> 32) return RPP_INVALID_ARGUMENT;  // positions are kept in 32 bits
  FrameHeader h;
  if (parse_frame_header(in, in_n, h) < 0) return RPP_CORRUPT_INPUT;
  if ((h.flags & kFlagContentSize) && h.content != out_n) return RPP_CORRUPT_INPUT;
  fr.window = (h.flags & kFlagSingleSegment) ? out_n : h.window;
  fr.block_max = uint32_t(fr.window < kBlockMax ? fr.window : kBlockMax);
  uint64_t at = h.bytes, lit_sum = 0, seq_sum = 0;
  uint32_t nb = 0, last_huf = kNone, last_tab[3] = {kNone, kNone, kNone};
  for (;;) {  // every turn passes at least the 3 bytes of a block header
    fr.nblocks = nb;
    if (at + 3 > in_n) return RPP_CORRUPT_INPUT;
    const uint32_t hd = uint32_t(rd_le(in + at, 3)), kind = hd >> 1 & 3, size = hd >> 3;
    const uint64_t held = kind == kRle ? 1 : size;
    if (kind == 3 || at + 3 + held > in_n || size > fr.block_max) return RPP_CORRUPT_INPUT;
    BlockRec r{};
    r.frame = frame;
    r.kind = kind;
    r.pos = uint32_t(at + 3);
    r.size = size;
    r.huf_src = kNone;
    r.status = RPP_OK;
    if (kind == kCompressed) {
      if (size < 3) return RPP_CORRUPT_INPUT;
      const uint8_t* body = in + at + 3;
      LiteralsHeader lh;
      SequencesHeader sh;
      if (parse_literals_header(body, size, lh) < 0) return RPP_CORRUPT_INPUT;
      const uint32_t lit_bytes = lh.bytes + lh.comp;
      if (parse_sequences_header(body + lit_bytes, size - lit_bytes, sh) < 0) return RPP_CORRUPT_INPUT;
      r.lit_kind = lh.kind;
      r.lit_hdr = lh.bytes;
      r.lit_regen = lh.regen;
      r.lit_comp = lh.comp;
      r.lit_streams = lh.streams;
      if (lh.kind == kLitCompressed) last_huf = nb;
      if (lh.kind >= kLitCompressed) {
        if (last_huf == kNone) return RPP_CORRUPT_INPUT;
        r.huf_src = last_huf;
      }
      r.seq_pos = r.pos + lit_bytes;
      r.seq_count = sh.count;
      r.seq_hdr = sh.bytes;
      r.modes = sh.modes;
      for (uint32_t k = 0; k < 3; ++k) {
        r.tab_src[k] = kNone;
        if (!sh.count) continue;
        if (table_mode(sh.modes, k) != kRepeat) last_tab[k] = nb;
        if (last_tab[k] == kNone) return RPP_CORRUPT_INPUT;
        r.tab_src[k] = last_tab[k];
      }
      // every literal and every match (3 bytes at least) is output: more of them than that is corrupt
      r.lit_at = uint32_t(lit_sum);
      r.seq_at = uint32_t(seq_sum);
      lit_sum += lh.regen;
      seq_sum += sh.count;
      if (lit_sum > out_n || 3 * seq_sum > out_n) return RPP_CORRUPT_INPUT;
    }
    if (recs && nb < cap) recs[nb] = r;
    if (++nb == kNone) return RPP_CORRUPT_INPUT;
    at += 3 + held;
    if (hd & 1) break;
  }
  fr.nblocks = nb;  // (all blocks are sound also where what follows them is not)
  if (at + ((h.flags & kFlagChecksum) ? 4 : 0) != in_n) return RPP_CORRUPT_INPUT;  // (the checksum is skipped)
  return RPP_OK;
}

__global__ __launch_bounds__(kIndexThreads) void rpp_zstd_index_kernel(
    const uint8_t* __restrict__ d_in, const uint64_t* __restrict__ in_offsets, const uint64_t* __restrict__ in_bytes,
    uint32_t nframes, const uint64_t* __restrict__ out_bytes, Ws ws) {
  for (uint32_t f = threadIdx.x; f < nframes; f += kIndexThreads) {
    FrameRec fr{};
    fr.status = walk_frame(d_in + in_offsets[f], in_bytes[f], out_bytes[f], f, fr, nullptr, 0);
    ws.frames[f] = fr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // slots frame by frame: a frame that does not fit takes none
    uint32_t base = 0;
    uint64_t lit = 0, seq = 0;
    // The valid frames first: the promise counts their blocks, and no corrupt frame's blocks may cost one of them
    // its slots.  Then, from what is left, a corrupt frame's blocks before the failing one, decoded like a valid
    // frame's; one that does not fit there keeps its status and nothing of it is decoded.
    for (uint32_t pass = 0; pass < 2; ++pass) {
      for (uint32_t f = 0; f < nframes; ++f) {
        FrameRec fr = ws.frames[f];
        if ((fr.status == RPP_OK) != (pass == 0)) continue;
        const uint64_t out_n = out_bytes[f];
        bool run = fr.status == RPP_OK || (fr.status == RPP_CORRUPT_INPUT && fr.nblocks > 0);
        if (run && (fr.nblocks > ws.max_blocks - base || out_n > ws.lit_cap - lit || out_n / 3 > ws.seq_cap - seq)) {
          if (fr.status == RPP_OK) fr.status = RPP_OUTPUT_TOO_SMALL;
          run = false;
        }
        if (run) {
          fr.block_base = base;
          fr.lit_base = lit;
          fr.seq_base = seq;
          base += fr.nblocks;
          lit += out_n;
          seq += out_n / 3;
        } else {
          fr.nblocks = 0;
        }
        ws.frames[f] = fr;
      }
    }
    *ws.used = base;
  }
  __syncthreads();
  for (uint32_t f = threadIdx.x; f < nframes; f += kIndexThreads) {
    FrameRec fr = ws.frames[f];
    if (fr.nblocks)
      walk_frame(d_in + in_offsets[f], in_bytes[f], out_bytes[f], f, fr, ws.blocks + fr.block_base, fr.nblocks);
  }
}

// ---------------------------------------------------------------------------
// entropy
// ---------------------------------------------------------------------------
struct WaveLds {
  uint16_t huf[1u << kHufLog];
  FseEntry ll[1u << kTableLog[0]], of[1u << kTableLog[1]], ml[1u << kTableLog[2]];
  int16_t freq[kFreqSlots];
  uint16_t next[kFreqSlots];
  uint8_t weights[kWeightSlots + 12];
};

// the three tables of block r and its sequences, by one lane
__device__ bool block_sequences(const uint8_t* fin, const BlockRec* fblocks, const BlockRec& r, WaveLds& L, Seq* out) {
  FseEntry* const tab[3] = {L.ll, L.of, L.ml};
  uint32_t log[3];
  for (uint32_t k = 0; k < 3; ++k) {
    const BlockRec& s = fblocks[r.tab_src[k]];
    const uint32_t mode = table_mode(s.modes, k);
    if (mode == kRepeat) return false;
    const uint8_t* sp = fin + s.seq_pos + s.seq_hdr;
    const uint64_t sn = uint64_t(s.pos) + s.size - (uint64_t(s.seq_pos) + s.seq_hdr);
    const int64_t at = table_position(s.modes, k, sp, sn, L.freq);
    if (at < 0 || table_setup(k, mode, sp + at, sn - uint64_t(at), tab[k], log[k], L.freq, L.next) < 0) return false;
  }
  const uint8_t* sp = fin + r.seq_pos + r.seq_hdr;
  const uint64_t sn = uint64_t(r.pos) + r.size - (uint64_t(r.seq_pos) + r.seq_hdr);
  const int64_t at = table_position(r.modes, 3, sp, sn, L.freq);  // behind the block's own descriptions
  if (at < 0 || uint64_t(at) >= sn) return false;
  return decode_sequences(sp + at, sn - uint64_t(at), L.ll, log[0], L.of, log[1], L.ml, log[2], r.seq_count, out);
}

__global__ __launch_bounds__(kWave* kEntropyWaves) void rpp_zstd_entropy_kernel(
    const uint8_t* __restrict__ d_in, const uint64_t* __restrict__ in_offsets, Ws ws) {
  __shared__ WaveLds lds[kEntropyWaves];
  __shared__ uint32_t tree[kEntropyWaves][3];  // ok, table log, bytes of the description
  const uint32_t wave = threadIdx.x / kWave, lane = lane_id(), g = blockIdx.x * kEntropyWaves + wave;
  WaveLds& L = lds[wave];
  // (no wave leaves before the barrier: one that has no block, or no Huffman literals, waits with the others)
  const bool has = g < *ws.used && ws.blocks[g].kind == kCompressed;
  BlockRec r{};
  FrameRec fr{};
  const uint8_t* fin = nullptr;
  const BlockRec* fblocks = nullptr;
  if (has) {
    r = ws.blocks[g];
    fr = ws.frames[r.frame];
    fin = d_in + in_offsets[r.frame];
    fblocks = ws.blocks + fr.block_base;
  }
  const bool huffman = has && r.lit_kind >= kLitCompressed;
  if (huffman && lane == 0) {
    const BlockRec& s = fblocks[r.huf_src];
    uint32_t count = 0, log = 0;
    const int used = huf_read_weights(fin + s.pos + s.lit_hdr, s.lit_comp, L.weights, count, L.ll, L.freq, L.next);
    tree[wave][0] = used >= 0 && huf_build(L.weights, count, L.huf, log);
    tree[wave][1] = log;
    tree[wave][2] = used < 0 ? 0 : uint32_t(used);
  }
  __syncthreads();
  if (!has) return;
  uint8_t* const lits = ws.lits + fr.lit_base + r.lit_at;
  const uint8_t* const body = fin + r.pos + r.lit_hdr;
  bool ok = true;
  if (r.lit_kind == kLitRaw) {
    wave_copy(lits, body, r.lit_regen, lane);
  } else if (r.lit_kind == kLitRle) {
    const uint8_t v = body[0];
    for (uint32_t j = lane; j < r.lit_regen; j += kWave) lits[j] = v;
  } else {
    ok = tree[wave][0] != 0;
    const uint32_t skip = r.lit_kind == kLitCompressed ? tree[wave][2] : 0;  // a Treeless section is all streams
    const uint8_t* streams = body + skip;
    const uint64_t n = r.lit_comp - skip;
    bool mine = true;
    if (ok && r.lit_streams == 1) {
      if (lane == 0) mine = n >= 1 && huf_decode_stream(L.huf, tree[wave][1], streams, n, lits, r.lit_regen);
    } else if (ok) {
      uint32_t at[4], bytes[4], cnt[4];
      mine = huf_four_streams(streams, n, r.lit_regen, at, bytes, cnt);
      if (mine && lane < 4)
        mine = huf_decode_stream(L.huf, tree[wave][1], streams + at[lane], bytes[lane], lits + lane * cnt[0], cnt[lane]);
    }
    ok = ok && __all(mine);
  }
  if (lane == 0) {
    if (ok && r.seq_count) ok = block_sequences(fin, fblocks, r, L, ws.seqs + fr.seq_base + r.seq_at);
    ws.blocks[g].status = ok ? RPP_OK : RPP_CORRUPT_INPUT;
  }
}

// ---------------------------------------------------------------------------
// execute
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void rpp_zstd_execute_kernel(
    const uint8_t* __restrict__ d_in, const uint64_t* __restrict__ in_offsets, uint32_t nframes, uint8_t* d_out,
    const uint64_t* __restrict__ out_offsets, const uint64_t* __restrict__ out_bytes, int32_t* __restrict__ d_status,
    Ws ws) {
  const uint32_t f = blockIdx.x, lane = lane_id();
  if (f >= nframes) return;
  const FrameRec fr = ws.frames[f];
  if (fr.nblocks == 0) {  // (a valid frame has a block at least)
    if (lane == 0) d_status[f] = fr.status;
    return;
  }
  const uint8_t* const fin = d_in + in_offsets[f];
  uint8_t* const dst = d_out + out_offsets[f];
  const uint64_t out_n = out_bytes[f];
  const uint8_t* const flits = ws.lits + fr.lit_base;
  const Seq* const fseqs = ws.seqs + fr.seq_base;
  uint32_t rep[3] = {1, 4, 8};
  uint64_t op = 0, flushed = 0;  // flushed: output below it was stored before the last wait
  bool bad = false;
  for (uint32_t b = 0; b < fr.nblocks && !bad; ++b) {
    const BlockRec r = ws.blocks[fr.block_base + b];
    if (r.kind != kCompressed) {
      if (r.size > out_n - op) { bad = true; break; }
      if (r.kind == kRaw) {
        wave_copy(dst + op, fin + r.pos, r.size, lane);
      } else {
        const uint8_t v = fin[r.pos];
        for (uint32_t j = lane; j < r.size; j += kWave) dst[op + j] = v;
      }
      op += r.size;
      continue;
    }
    if (r.status != RPP_OK) { bad = true; break; }
    const uint8_t* const lits = flits + r.lit_at;
    const uint64_t start = op;
    uint32_t lit_at = 0;
    for (uint32_t t = 0; t < r.seq_count && !bad; t += kWave) {
      const uint32_t here = min(r.seq_count - t, kWave);
      Seq q{0, 0, 0};
      if (lane < here) q = fseqs[r.seq_at + t + lane];
      for (uint32_t j = 0; j < here; ++j) {
        const uint32_t ll = __shfl(q.ll, int(j)), ml = __shfl(q.ml, int(j)), ov = __shfl(q.ov, int(j));
        if (ll > r.lit_regen - lit_at) { bad = true; break; }
        const uint32_t off = resolve_offset(rep, ll, ov);
        const uint64_t len = uint64_t(ll) + ml;
        if (len > fr.block_max - (op - start) || len > out_n - op) { bad = true; break; }
        wave_copy(dst + op, lits + lit_at, ll, lane);
        lit_at += ll;
        op += ll;
        if (off == 0 || off > op || off > fr.window) { bad = true; break; }
        const uint8_t* const from = dst + op - off;
        const uint64_t span = ml < off ? ml : off;  // the source bytes the match reads
        if (op - off + span > flushed) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have landed
          flushed = op;
        }
        if (off >= ml) {
          wave_copy(dst + op, from, ml, lane);
        } else {  // a pattern of `off` bytes repeated
          uint32_t at = lane % off;
          const uint32_t adv = kWave % off;
          for (uint32_t i = lane; i < ml; i += kWave) {
            dst[op + i] = from[at];
            at += adv;
            if (at >= off) at -= off;
          }
        }
        op += ml;
      }
    }
    if (bad) break;
    const uint32_t rest = r.lit_regen - lit_at;
    if (rest > fr.block_max - (op - start) || rest > out_n - op) { bad = true; break; }
    wave_copy(dst + op, lits + lit_at, rest, lane);
    op += rest;
  }
  if (lane == 0) d_status[f] = fr.status == RPP_OK && !bad && op == out_n ? RPP_OK : RPP_CORRUPT_INPUT;
}

uint64_t align16(uint64_t v) { return (v + 15) & ~UINT64_C(15); }

uint64_t fixed_bytes(uint32_t max_blocks) {
  return 16 + align16(sizeof(FrameRec) * uint64_t(max_blocks)) + align16(sizeof(BlockRec) * uint64_t(max_blocks));
}

}  // namespace

// 15 bytes per sequence record the batch can hold: the record itself (12) and 3 literal bytes
extern "C" uint64_t rpp_zstd_decode_workspace_bytes(uint64_t total_out_bytes, uint32_t max_blocks) {
  return fixed_bytes(max_blocks) + 15 * (total_out_bytes / 3 + kSlack);
}

extern "C" int rpp_zstd_decode_batch(const uint8_t* d_in, const uint64_t* d_in_offsets, const uint64_t* d_in_bytes,
                                     uint32_t nframes, uint8_t* d_out, const uint64_t* d_out_offsets,
                                     const uint64_t* d_out_bytes, int32_t* d_status, uint32_t max_blocks,
                                     void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (nframes == 0) return RPP_OK;
  if (!d_in || !d_in_offsets || !d_in_bytes || !d_out || !d_out_offsets || !d_out_bytes || !d_status ||
      !d_workspace || ((uintptr_t)d_workspace & 15))
    return RPP_INVALID_ARGUMENT;
  // a frame has a block at least, so a promise below the number of frames cannot hold
  if (max_blocks < nframes || workspace_bytes < rpp_zstd_decode_workspace_bytes(0, max_blocks))
    return RPP_OUTPUT_TOO_SMALL;
  uint8_t* p = static_cast<uint8_t*>(d_workspace);
  Ws ws{};
  ws.used = reinterpret_cast<uint32_t*>(p);
  p += 16;
  ws.frames = reinterpret_cast<FrameRec*>(p);
  p += align16(sizeof(FrameRec) * uint64_t(max_blocks));
  ws.blocks = reinterpret_cast<BlockRec*>(p);
  p += align16(sizeof(BlockRec) * uint64_t(max_blocks));
  ws.seq_cap = (workspace_bytes - fixed_bytes(max_blocks)) / 15;
  ws.lit_cap = 3 * ws.seq_cap;
  ws.seqs = reinterpret_cast<Seq*>(p);
  ws.lits = p + sizeof(Seq) * ws.seq_cap;
  ws.max_blocks = max_blocks;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rpp_zstd_index_kernel, dim3(1), dim3(kIndexThreads), 0, s, d_in, d_in_offsets, d_in_bytes, nframes,
                     d_out_bytes, ws);
  hipLaunchKernelGGL(rpp_zstd_entropy_kernel, dim3((max_blocks + kEntropyWaves - 1) / kEntropyWaves),
                     dim3(kWave * kEntropyWaves), 0, s, d_in, d_in_offsets, ws);
  hipLaunchKernelGGL(rpp_zstd_execute_kernel, dim3(nframes), dim3(kWave), 0, s, d_in, d_in_offsets, nframes, d_out,
                     d_out_offsets, d_out_bytes, d_status, ws);
  return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR;
}
