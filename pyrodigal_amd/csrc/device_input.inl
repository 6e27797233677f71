// Sequences that already lie in device memory (pga_batch_create_device; the rule is in pyrodigal_amd.h).
// Included by finder.hip: no separate translation unit, the batch code's statics are shared.
//
// One kernel gathers ragged or padded rows of 1-, 4- or 8-byte elements, maps token ids to letters and writes the packed ASCII
// layout that k_digitize and the renderers read; everything behind the batch is the code every other batch runs.

constexpr int kPackThreads = 256;

// f(e) of the rule: the range test comes first, so an id outside the table is a compare and never an address
__device__ __forceinline__ uint32_t pack_letter(const int64_t e, const uint8_t* s_alpha, const int n_alpha) {
    return (uint64_t)e < (uint64_t)n_alpha ? (uint32_t)s_alpha[e] : (uint32_t)'N';
}
template <int EB>
__device__ __forceinline__ int64_t pack_elem(const void* __restrict__ src, const int64_t k) {
    if (EB == 1) return (int64_t)reinterpret_cast<const uint8_t*>(src)[k];
    if (EB == 4) return (int64_t)reinterpret_cast<const int32_t*>(src)[k];
    return reinterpret_cast<const int64_t*>(src)[k];
}
// the letters of one 16-byte piece of the source, lowest address in the lowest byte: 4 of 4-byte elements, 2 of 8-byte ones
template <int EB>
__device__ __forceinline__ uint32_t pack_piece(const uint4 v, const uint8_t* s_alpha, const int n_alpha) {
    if (EB == 4)
        return pack_letter((int64_t)(int32_t)v.x, s_alpha, n_alpha) | (pack_letter((int64_t)(int32_t)v.y, s_alpha, n_alpha) << 8) |
               (pack_letter((int64_t)(int32_t)v.z, s_alpha, n_alpha) << 16) | (pack_letter((int64_t)(int32_t)v.w, s_alpha, n_alpha) << 24);
    return pack_letter((int64_t)((uint64_t)v.x | ((uint64_t)v.y << 32)), s_alpha, n_alpha) |
           (pack_letter((int64_t)((uint64_t)v.z | ((uint64_t)v.w << 32)), s_alpha, n_alpha) << 8);
}
__device__ __forceinline__ uint32_t pack_word(const uint32_t w, const uint8_t* s_alpha, const int n_alpha) {
    return pack_letter((int64_t)(w & 255u), s_alpha, n_alpha) | (pack_letter((int64_t)((w >> 8) & 255u), s_alpha, n_alpha) << 8) |
           (pack_letter((int64_t)((w >> 16) & 255u), s_alpha, n_alpha) << 16) | (pack_letter((int64_t)(w >> 24), s_alpha, n_alpha) << 24);
}

// Work is dealt by destination bytes, as in k_circ_rotate: a thread owns 16 consecutive bytes of the packed letters (the allocation is
// 256-byte aligned) and finds its contig by binary search in the destination bases, so one 200 Mbp contig and 100 000 short ones both
// fill the device.  Contig j's letters are the elements soff[j] .. soff[j] + dct[j].len of `src`; nothing else of `src` is read.
//   * 16 letters of one contig: one aligned 16-byte store.  1-byte elements: one 16-byte load at whatever alignment the source has.
//     4- and 8-byte elements, when the 1024 letters of a wavefront come from one contig: 4 (8) load instructions, each of which
//     reads 1024 contiguous bytes across the wavefront (lane l of load k takes piece 64 k + l); a lane turns its piece into 4 (2)
//     letters, puts them at their place in 1 KB of LDS of the wavefront, and then reads back the 16 letters it owns.  Otherwise
//     the thread loads its own 64 (128) bytes in 16-byte pieces.
//   * threads on a seam between contigs, and the last of the batch, go letter by letter; empty contigs are stepped over.
//   * the bytes [total, total + 16) get 'N': the batch's bytes do not depend on what the allocation held before.
// TABLE: the letters come through the alphabet, staged once per workgroup in 256 bytes of LDS (the indices diverge per lane, so it is
// neither a constant nor a scalar table; entries from n_alpha on are 'N' and never read).  The 1-byte form without one copies.
template <int EB, bool TABLE>
__global__ void __launch_bounds__(kPackThreads)
k_pack_device(const void* __restrict__ src, const ContigDesc* __restrict__ dct, const int64_t* __restrict__ soff, const int n, const int64_t total,
              const uint8_t* __restrict__ alpha, const int n_alpha, char* __restrict__ dst) {
    static_assert(EB == 1 || EB == 4 || EB == 8, "element width");
    static_assert(TABLE || EB == 1, "only bytes can be letters themselves");
    __shared__ uint8_t s_alpha[256];
    __shared__ __attribute__((aligned(16))) char s_wave[EB > 1 ? (kPackThreads / 64) * 1024 : 16];
    if (TABLE) { s_alpha[threadIdx.x] = alpha[threadIdx.x]; __syncthreads(); }
    const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (q0 >= total + 16) return;
    const int64_t q1 = q0 + 16 < total ? q0 + 16 : total;       // (<= q0 for a thread that only writes padding)
    int j = 0;
    ContigDesc d{0, 0, 0};
    bool whole = false;                                          // the 16 letters come from one contig
    if (q0 < total) {
        int lo = 0, hi = n - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (dct[mid].base <= q0) lo = mid; else hi = mid - 1; }
        j = lo;
        d = dct[j];
        whole = q1 - q0 == 16 && q0 - d.base + 16 <= d.len;
    }
    if (EB > 1) {
        // (a lane that has left, or that writes padding, sits in the wavefront of the batch's last letters: `whole` fails there)
        const int lane = threadIdx.x & 63;
        const int j0 = __shfl(j, 0);
        if (__all(whole && j == j0)) {
            char* wb = s_wave + (threadIdx.x >> 6) * 1024;
            const char* sp = reinterpret_cast<const char*>(src) + (soff[j] + (q0 - (int64_t)lane * 16 - d.base)) * EB;
#pragma unroll
            for (int k = 0; k < EB; k++) {
                uint4 v;
                __builtin_memcpy(&v, sp + (size_t)(k * 64 + lane) * 16, 16);
                const uint32_t w = pack_piece<EB>(v, s_alpha, n_alpha);
                if (EB == 4) *reinterpret_cast<uint32_t*>(wb + (k * 64 + lane) * 4) = w;
                else *reinterpret_cast<uint16_t*>(wb + (k * 64 + lane) * 2) = (uint16_t)w;
            }
            // the wavefront's own LDS: its writes above are visible to its reads below
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            *reinterpret_cast<uint4*>(dst + q0) = *reinterpret_cast<const uint4*>(wb + lane * 16);
            return;
        }
    }
    if (whole) {
        const char* sp = reinterpret_cast<const char*>(src) + (soff[j] + (q0 - d.base)) * EB;
        uint4 o;
        if (EB == 1) {
            __builtin_memcpy(&o, sp, 16);
            if (TABLE) { o.x = pack_word(o.x, s_alpha, n_alpha); o.y = pack_word(o.y, s_alpha, n_alpha); o.z = pack_word(o.z, s_alpha, n_alpha); o.w = pack_word(o.w, s_alpha, n_alpha); }
        } else if (EB == 4) {
            uint4 v;
            __builtin_memcpy(&v, sp, 16);      o.x = pack_piece<EB>(v, s_alpha, n_alpha);
            __builtin_memcpy(&v, sp + 16, 16); o.y = pack_piece<EB>(v, s_alpha, n_alpha);
            __builtin_memcpy(&v, sp + 32, 16); o.z = pack_piece<EB>(v, s_alpha, n_alpha);
            __builtin_memcpy(&v, sp + 48, 16); o.w = pack_piece<EB>(v, s_alpha, n_alpha);
        } else {
            uint4 v, u;
            __builtin_memcpy(&v, sp, 16);      __builtin_memcpy(&u, sp + 16, 16);  o.x = pack_piece<EB>(v, s_alpha, n_alpha) | (pack_piece<EB>(u, s_alpha, n_alpha) << 16);
            __builtin_memcpy(&v, sp + 32, 16); __builtin_memcpy(&u, sp + 48, 16);  o.y = pack_piece<EB>(v, s_alpha, n_alpha) | (pack_piece<EB>(u, s_alpha, n_alpha) << 16);
            __builtin_memcpy(&v, sp + 64, 16); __builtin_memcpy(&u, sp + 80, 16);  o.z = pack_piece<EB>(v, s_alpha, n_alpha) | (pack_piece<EB>(u, s_alpha, n_alpha) << 16);
            __builtin_memcpy(&v, sp + 96, 16); __builtin_memcpy(&u, sp + 112, 16); o.w = pack_piece<EB>(v, s_alpha, n_alpha) | (pack_piece<EB>(u, s_alpha, n_alpha) << 16);
        }
        *reinterpret_cast<uint4*>(dst + q0) = o;
        return;
    }
    for (int64_t q = q0; q < q1; q++) {
        while (q >= d.base + d.len) { j++; d = dct[j]; }         // (empty contigs are stepped over; q < total ends it)
        const int64_t e = pack_elem<EB>(src, soff[j] + (q - d.base));
        dst[q] = TABLE ? (char)pack_letter(e, s_alpha, n_alpha) : (char)e;
    }
    for (int64_t q = q0 > total ? q0 : total; q < q0 + 16 && q < total + 16; q++) dst[q] = 'N';
}

// what the kernel reads per contig, behind the tile tables in the batch's allocation (256-byte aligned): the destination ContigDescs
// (n + 1), the source offsets (n) and the alphabet padded to 256 bytes
static size_t pack_tables_bytes(int n) { return sizeof(ContigDesc) * ((size_t)n + 1) + sizeof(int64_t) * (size_t)n + 256 + 256; }

int pga_device_memory_(pga_ctx* c, const void* p, const char* fn, const char* name) {
    hipPointerAttribute_t at{};
    const hipError_t pe = p ? hipPointerGetAttributes(&at, p) : hipErrorInvalidValue;
    if (pe != hipSuccess) (void)hipGetLastError();
    if (pe == hipSuccess && at.type == hipMemoryTypeDevice && at.device == c->device) return PGA_OK;
    c->err = std::string(fn) + ": " + name + " is not device memory";
    if (pe != hipSuccess || at.type != hipMemoryTypeDevice) c->err += " (a host pointer?)";
    else c->err += " of the context's device " + std::to_string(c->device) + " but of device " + std::to_string(at.device);
    return PGA_EINVAL;
}

extern "C" int pga_batch_create_device(pga_ctx* c, int32_t n_contigs, const void* d_data, int64_t n_elems, int32_t elem_bytes,
                                       const int64_t* elem_off, const int64_t* lens, const uint8_t* alphabet, int32_t n_alphabet,
                                       void* producer_stream, pga_batch** out) {
    if (out) *out = nullptr;
    if (!c) return PGA_EINVAL;
    if (!out || n_contigs < 0 || n_elems < 0 || (n_contigs > 0 && (!elem_off || !lens))) { c->err = "pga_batch_create_device: bad arguments"; return PGA_EINVAL; }
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) {
        c->err = "pga_batch_create_device: elem_bytes must be 1, 4 or 8, not " + std::to_string(elem_bytes); return PGA_EINVAL;
    }
    if (!alphabet && n_alphabet != 0) { c->err = "pga_batch_create_device: n_alphabet without an alphabet"; return PGA_EINVAL; }
    if (!alphabet && elem_bytes != 1) {
        c->err = "pga_batch_create_device: elements of " + std::to_string(elem_bytes) + " bytes are token ids and need an alphabet"; return PGA_EINVAL;
    }
    if (alphabet) {
        if (n_alphabet < 0 || n_alphabet > 256) { c->err = "pga_batch_create_device: n_alphabet must be 0 .. 256, not " + std::to_string(n_alphabet); return PGA_EINVAL; }
        for (int k = 0; k < n_alphabet; k++) {
            const uint8_t a = alphabet[k];
            if (!((a >= 'A' && a <= 'Z') || (a >= 'a' && a <= 'z'))) {
                c->err = "pga_batch_create_device: alphabet entry " + std::to_string(k) + " (byte " + std::to_string((int)a) + ") is not an ASCII letter"; return PGA_EINVAL;
            }
        }
    }
    int64_t total = 0;
    for (int i = 0; i < n_contigs; i++) {
        if (lens[i] < 0 || lens[i] > 0x7fff0000LL) { c->err = "pga_batch_create_device: contig " + std::to_string(i) + ": bad contig length " + std::to_string(lens[i]); return PGA_EINVAL; }
        if (elem_off[i] < 0 || elem_off[i] > n_elems || lens[i] > n_elems - elem_off[i]) {
            c->err = "pga_batch_create_device: contig " + std::to_string(i) + ": elements [" + std::to_string(elem_off[i]) + ", " + std::to_string(elem_off[i]) + " + " +
                     std::to_string(lens[i]) + ") do not lie in the " + std::to_string(n_elems) + " elements of the data";
            return PGA_EINVAL;
        }
        total += lens[i];
        if (total >= 0x7fffffffLL) { c->err = "pga_batch_create_device: batch larger than 2^31 bases; split it"; return PGA_EINVAL; }
    }
    HT(c, hipSetDevice(c->device));
    if (total > 0) { const int rc = pga_device_memory_(c, d_data, "pga_batch_create_device", "d_data"); if (rc) return rc; }
    if (!c->finder) { int rc = pga_finder_models_changed(c); if (rc) return rc; }
    pga_batch* b = new (std::nothrow) pga_batch();
    if (!b) return PGA_ENOMEM;
    b->ctx = c; b->n = n_contigs; b->d_seq = nullptr; b->d_tiles = nullptr; b->d_tile0 = nullptr; b->n_tiles = 0; b->ct.resize((size_t)n_contigs + 1);
    total = 0;
    for (int i = 0; i < n_contigs; i++) { b->ct[i].base = total; b->ct[i].len = (int32_t)lens[i]; b->ct[i]._pad = 0; total += lens[i]; }
    b->ct[n_contigs].base = total; b->ct[n_contigs].len = 0; b->ct[n_contigs]._pad = 0;
    b->total = total;
    if (total > 0) {
        FinderState* f = c->finder;
        std::lock_guard<std::mutex> up(f->up_mu);                 // one upload at a time per context; a call of the context may run beside it
        const size_t n = (size_t)n_contigs, tab = pack_tables_bytes(n_contigs);
        hipStream_t st = nullptr; char* h_tab = nullptr;
        { const int rc = upload_resources(c, tab, &st, &h_tab); if (rc) { delete b; return rc; } }
        if (!f->up_ev) { const int rc = pga_hip_try_(c, hipEventCreateWithFlags(&f->up_ev, hipEventDisableTiming), "hipEventCreate"); if (rc) { delete b; return rc; } }
        std::vector<TileDesc> tiles; std::vector<int32_t> tile0;
        batch_tiles(b, tiles, tile0);
        const size_t tiles_b = batch_tiles_bytes(tiles, tile0);
        if (batch_take_dev(c, (size_t)total + 16 + tiles_b + tab, &b->d_seq, &b->d_seq_cap) != hipSuccess) { delete b; c->err = "pga_batch_create_device: hipMalloc failed"; return PGA_ENOMEM; }
        // the kernel's tables, in the pinned staging area as they will lie on the device
        const size_t dct_b = sizeof(ContigDesc) * (n + 1), off_b = sizeof(int64_t) * n;
        memcpy(h_tab, b->ct.data(), dct_b);
        memcpy(h_tab + dct_b, elem_off, off_b);
        memset(h_tab + dct_b + off_b, 'N', 256);
        if (n_alphabet > 0) memcpy(h_tab + dct_b + off_b, alphabet, (size_t)n_alphabet);
        char* d_tab = (char*)(((uintptr_t)(b->d_seq + total + 16 + tiles_b) + 255) & ~(uintptr_t)255);
        // the upload stream is non-blocking: it waits for what the producer's stream held when the call came
        hipError_t e = hipEventRecord(f->up_ev, (hipStream_t)producer_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, f->up_ev, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tab, h_tab, dct_b + off_b + 256, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = batch_upload_tiles(b, b->d_seq + total + 16, tiles, tile0, st);
        if (e == hipSuccess) {
            const ContigDesc* d_dct = (const ContigDesc*)d_tab;
            const int64_t* d_off = (const int64_t*)(d_tab + dct_b);
            const uint8_t* d_alpha = (const uint8_t*)(d_tab + dct_b + off_b);
            const dim3 grid((unsigned)(((total + 16 + 15) / 16 + kPackThreads - 1) / kPackThreads)), block(kPackThreads);
            if (elem_bytes == 1 && !alphabet) hipLaunchKernelGGL((k_pack_device<1, false>), grid, block, 0, st, d_data, d_dct, d_off, n_contigs, total, d_alpha, 0, b->d_seq);
            else if (elem_bytes == 1) hipLaunchKernelGGL((k_pack_device<1, true>), grid, block, 0, st, d_data, d_dct, d_off, n_contigs, total, d_alpha, n_alphabet, b->d_seq);
            else if (elem_bytes == 4) hipLaunchKernelGGL((k_pack_device<4, true>), grid, block, 0, st, d_data, d_dct, d_off, n_contigs, total, d_alpha, n_alphabet, b->d_seq);
            else hipLaunchKernelGGL((k_pack_device<8, true>), grid, block, 0, st, d_data, d_dct, d_off, n_contigs, total, d_alpha, n_alphabet, b->d_seq);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);       // on return the source may be overwritten or freed
        if (e != hipSuccess) { batch_give_dev(c, b->d_seq, b->d_seq_cap); delete b; return pga_hip_try_(c, e, "packing of the device batch"); }
    }
    *out = b;
    return PGA_OK;
}

extern "C" int pga_batch_read(pga_ctx* c, const pga_batch* b, int32_t contig, char* out) {
    if (!c) return PGA_EINVAL;
    if (!b || b->ctx != c) { c->err = "pga_batch_read: bad arguments"; return PGA_EINVAL; }
    if (contig < -1 || contig >= b->n) { c->err = "pga_batch_read: contig " + std::to_string(contig) + " of a batch of " + std::to_string(b->n); return PGA_EINVAL; }
    const int64_t from = contig < 0 ? 0 : b->ct[contig].base, bytes = contig < 0 ? b->total : (int64_t)b->ct[contig].len;
    if (bytes == 0) return PGA_OK;
    if (!out) { c->err = "pga_batch_read: no buffer"; return PGA_EINVAL; }
    HT(c, hipSetDevice(c->device));
    std::lock_guard<std::mutex> up(c->finder->up_mu);
    hipStream_t st = nullptr;
    { const int rc = upload_resources(c, 0, &st, nullptr); if (rc) return rc; }
    HT(c, hipMemcpyAsync(out, b->d_seq + from, (size_t)bytes, hipMemcpyDeviceToHost, st));
    HT(c, hipStreamSynchronize(st));
    return PGA_OK;
}
