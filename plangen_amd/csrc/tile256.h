// The 256x256x64 bf16 MFMA tile pipeline for gfx950: eight waves (2 wave rows x 4 wave columns, 128x64 of C each), 128 KiB of LDS staging,
// one block per CU.  Used by gemm256.hip (persistent GEMM) and by the two fused scoring heads (score_head.hip, score_cfg_head.hip); this
// header holds the ONE copy of the staging stream, the counted waits and the barriers, and the invariants they rely on:
//
// * A K tile (64 wide) is staged as FOUR 16 KiB half-tiles named after the C quadrant that consumes them, not after their position in memory:
//       HA0 = A rows {wr*128 + [0,64)}      (m-tiles 0-3 of every wave)
//       HB0 = W rows {wc*64  + [0,32)}      (n-tiles 0-1 of every wave)
//       HB1 = W rows {wc*64  + 32 + [0,32)} (n-tiles 2-3)
//       HA1 = A rows {wr*128 + 64 + [0,64)} (m-tiles 4-7; a user with MT1 < 4 reads only the first 16 MT1 rows of it)
//   Every wave owns 128x64 of C = 8 x 4 MFMA tiles (mfma_f32_16x16x32_bf16) and walks its four 64x32 quadrants in the order (0,0) (0,1) (1,1) (1,0).
// * Two LDS buffers (even / odd K tile), each [HA0 | HA1 | HB0 | HB1].  The global_load_lds stream is "tile after tile, halves in the order
//   HA0 HB0 HB1 HA1", two loads per thread and half-tile, running more than one whole K tile ahead of its consumer; the loop never waits for
//   vmcnt(0).  K tiles past the end are staged from the last valid tile (never read): the loop is branch-free and the vmcnt counts stay exact.
//   prologue() issues tile 0 and HA0 HB0 of tile 1.
// * TWO-PHASE FORM (run()): phase A reads HB0, HA0, HB1 (quadrants (0,0) (0,1), 32 MFMAs) and stages HB1(kt+1), HA1(kt+1); phase B reads HA1
//   (quadrants (1,1) (1,0), 8 MT1 MFMAs; HB0 / HB1 stay in registers) and stages HA0(kt+2), HB0(kt+2).
//   Every phase = [ds_read fragments, issue 4 global_load_lds, counted vmcnt, lgkmcnt(0)] s_barrier [MFMAs under s_setprio 1] s_barrier.
//   RAW: phase B's load section ends with vmcnt(6) (HB1(kt+1) and everything older landed; the three half-tiles issued behind it are in
//   flight), phase A's with vmcnt(8) (HA1(kt) landed; four younger); both one full phase (two barriers) before the fragments are read.
//   WAR: a slot is re-staged in the phase RIGHT AFTER the one that read it (HA0 / HB0: read A(kt), staged B(kt); HA1: read B(kt), staged
//   A(kt+1); HB1: read A(kt), staged A(kt+1)).  Every wave executes `s_waitcnt lgkmcnt(0)` BEFORE the barrier that ends its load section (its
//   fragments are in registers when it arrives), so one barrier separates the last read of a slot from any global_load_lds into it.
//   tools/dma_isa_check.py replays both rules on the compiled code: a re-stage needs >= 2 barriers since the slot's last read, or 1 barrier
//   with the read drained in front of it.
// * One-barrier stagger: waves with wr == 1 pass one extra barrier before the loop (open()) and the others one behind it (close()), so on
//   every SIMD one wave is in its MFMA section while the other one is in its load section: LDS reads and address arithmetic hide under the
//   other wave's MFMAs.  The RAW and WAR margins above hold with the two wave groups running one barrier apart; with the groups apart the
//   LEADING group issues a re-stage right behind the very barrier that ends the LAGGING group's load section, which is why the lgkmcnt(0)
//   drain sits in front of that barrier.
// * Behind close() every wave is past its last ds_read: a user may issue the next tile's prologue() before it consumes the accumulators
//   (loads return in order among themselves, and the clamped tail stages of this tile were issued earlier by the same wave to the same LDS
//   bytes).  drain() before the block touches the staging bytes for anything else, or ends.
//
// The A side goes through a loader (gemm_common.h: init(slot, row), set_ktile(k0), ptr(slot, k)) with four staging slots; slot_wr() / slot_row()
// name the tile row of each slot.  The W side is four row pointers clamped at N - 1 (set_W).
#pragma once
#include "gemm_common.h"

constexpr int T256_BK = 64;                              // K step
constexpr int T256_AH = 2 * 64 * 128;                    // bytes per A half-tile (2 wave rows x 64 rows x 128 B)
constexpr int T256_BH = 4 * 32 * 128;                    // bytes per W half-tile (4 wave columns x 32 rows x 128 B)
constexpr int T256_BUF = 2 * T256_AH + 2 * T256_BH;      // one K tile: [HA0 | HA1 | HB0 | HB1]
constexpr int T256_STAGING = 2 * T256_BUF;               // staging bytes of a block

// A loader whose four slots are row pointers the kernel gathered itself (the scoring heads' row_idx / cond_idx / uncond_idx).  ptr() adds the
// K tile base (wave-uniform, from set_ktile as in ConvLoaderS) before the thread's chunk offset: row + k0 + (k - k0), not row + k -- the 64-bit
// lane part of the address is then loop-invariant and only a scalar offset is added per K tile
struct GatherLoader {
    const bf16* rowp[4];
    int k0;
    __device__ __forceinline__ void init(int i, const bf16* row) { rowp[i] = row; }
    __device__ __forceinline__ void set_ktile(int k0_) { k0 = k0_; }
    __device__ __forceinline__ const bf16* ptr(int i, int k) const { return rowp[i] + k0 + (k - k0); }
};

template <class AL>
struct Tile256 {
    AL& al;
    char* const smem;
    const int nk;
    int srow, sc;                                        // staging: LDS row (+ i*64) and swizzled SOURCE chunk (elements) of this thread
    char* swave;
    int wr, wc, g, lr;                                   // wave row / column, lane group and lane row of the MFMA layout
    int aoff0, aoff1, boff0, boff1;                      // fragment addresses of k-steps 0 / 1 inside a buffer
    const bf16* wrow[4];

    __device__ __forceinline__ Tile256(AL& al_, char* smem_, int K) : al(al_), smem(smem_), nk(K / T256_BK) {
        const int l = threadIdx.x & 63;
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        // staging: wave w, instruction i covers LDS rows (i*8 + w)*8 .. +7 of a half-tile; the swizzle term (row>>1)&7 = (w&1)*4 + (l>>4) does not depend on i
        srow = w * 8 + (l >> 3);
        sc = ((l & 7) ^ (((w & 1) << 2) + (l >> 4))) * 8;
        swave = smem + w * 1024;
        wr = w >> 2; wc = w & 3; g = l >> 4; lr = l & 15;
        // fragment addresses: row*128 + ((ks*4+g) ^ ((row>>1)&7))*16; (row>>1)&7 == (lr>>1)&7 for every tile of this lane
        const int swz = (lr >> 1) & 7;
        aoff0 = (wr * 64 + lr) * 128 + ((g ^ swz) << 4); aoff1 = aoff0 ^ 64;
        boff0 = 2 * T256_AH + (wc * 32 + lr) * 128 + ((g ^ swz) << 4); boff1 = boff0 ^ 64;
    }

    static __device__ __forceinline__ void barrier() { asm volatile("s_barrier" ::: "memory"); }
    // counted wait: everything but the YOUNGER most recently issued half-tiles (2 loads each) has landed
    template <int YOUNGER> static __device__ __forceinline__ void wait_all_but() {
        static_assert(YOUNGER == 3 || YOUNGER == 4, "the schedules wait on 3 or 4 half-tiles in flight");
        if constexpr (YOUNGER == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    }
    static __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }      // clamped tail stages must not outlive the block's LDS

    // A staging slot s = h*2 + i of this thread brings row slot_row(s) (0..127: half h, 64 rows each) of wave row slot_wr(s)
    __device__ __forceinline__ int slot_wr(int s) const { return ((s & 1) * 64 + srow) >> 6; }
    __device__ __forceinline__ int slot_row(int s) const { return (s >> 1) * 64 + (((s & 1) * 64 + srow) & 63); }
    // W rows of half h of the column tile at n0; rows past the matrix re-read row N - 1
    __device__ __forceinline__ void set_W_half(int h, const bf16* W, long ldb, int n0, int N) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = i * 64 + srow;                 // LDS row of the half-tile
            const int n = n0 + (r >> 5) * 64 + h * 32 + (r & 31);
            wrow[h * 2 + i] = W + (long)(n < N ? n : N - 1) * ldb;
        }
    }
    __device__ __forceinline__ void set_W(const bf16* W, long ldb, int n0, int N) { set_W_half(0, W, ldb, n0, N); set_W_half(1, W, ldb, n0, N); }
    template <int H> __device__ __forceinline__ void stage_A(int T) {
        const int k0 = (T < nk ? T : nk - 1) * T256_BK;
        char* d = swave + (T & 1) * T256_BUF + H * T256_AH;
        al.set_ktile(k0);
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(al.ptr(H * 2 + i, k0 + sc), d + i * 8192);
    }
    template <int H> __device__ __forceinline__ void stage_B(int T) {
        const int k0 = (T < nk ? T : nk - 1) * T256_BK;
        char* d = swave + (T & 1) * T256_BUF + 2 * T256_AH + H * T256_BH;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(wrow[H * 2 + i] + k0 + sc, d + i * 8192);
    }
    // tile 0 complete + the first two halves of tile 1, in stream order
    __device__ __forceinline__ void prologue() { stage_A<0>(0); stage_B<0>(0); stage_B<1>(0); stage_A<1>(0); stage_A<0>(1); stage_B<0>(1); }

    // fragments of half-tile HA<H> (NM m-tiles) / HB<H> of the K tile in `buf`
    template <int H, int NM> __device__ __forceinline__ void read_A(const char* buf, bf16x8 (&a)[4][2]) const {
#pragma unroll
        for (int mt = 0; mt < NM; ++mt) {
            a[mt][0] = *(const bf16x8*)(buf + H * T256_AH + aoff0 + mt * 2048);
            a[mt][1] = *(const bf16x8*)(buf + H * T256_AH + aoff1 + mt * 2048);
        }
    }
    template <int H> __device__ __forceinline__ void read_B(const char* buf, bf16x8 (&b)[2][2]) const {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            b[nt][0] = *(const bf16x8*)(buf + H * T256_BH + boff0 + nt * 2048);
            b[nt][1] = *(const bf16x8*)(buf + H * T256_BH + boff1 + nt * 2048);
        }
    }

    // start of a tile: accumulators zeroed, the half-tiles the first phase reads retired, the second wave group one barrier behind
    template <int YOUNGER, int NMT> __device__ __forceinline__ void open(f32x4 (&acc)[NMT][4]) const {
#pragma unroll
        for (int i = 0; i < NMT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wait_all_but<YOUNGER>();
        barrier();
        if (wr >= 1) barrier();
    }
    __device__ __forceinline__ void close() const { if (wr < 1) barrier(); }

    // MFMA section of the two-phase form: row half MH against both column halves.  Operands swapped (W fragment first): D rows = n,
    // D cols = m, so a lane holds 4 CONSECUTIVE columns n = g*4 .. +3 of row m = lr -> one 16-byte store per MFMA tile in an epilogue
    template <int MH, int NHA, int NHB, int NMT>
    static __device__ __forceinline__ void mfma_section2(f32x4 (&acc)[NMT][4], const bf16x8 (&a)[4][2], const bf16x8 (&bfa)[2][2], const bf16x8 (&bfb)[2][2]) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // WAR: fragments in registers BEFORE the barrier, see the header
        barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < (MH ? NMT - 4 : 4); ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc[MH * 4 + mt][NHA * 2 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfa[nt][ks], a[mt][ks], acc[MH * 4 + mt][NHA * 2 + nt], 0, 0, 0);
                    acc[MH * 4 + mt][NHB * 2 + nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfb[nt][ks], a[mt][ks], acc[MH * 4 + mt][NHB * 2 + nt], 0, 0, 0);
                }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        barrier();
    }

    // One tile on the two-phase schedule: acc = A tile . W tile^T over all nk K tiles.  Needs prologue() issued (and nothing else in flight
    // behind it); leaves the clamped tail stages in flight.  NMT = 4 + MT1 m-tiles per wave (MT1 = m-tiles of the second row half).
    template <int NMT> __device__ __forceinline__ void run(f32x4 (&acc)[NMT][4]) {
        static_assert(NMT >= 5 && NMT <= 8, "second row half: 1..4 m-tiles");
        bf16x8 a[4][2], b0[2][2], b1[2][2];
        open<3>(acc);                                           // HB1(0) landed (younger: HA1(0) HA0(1) HB0(1))
        for (int kt = 0; kt < nk; ++kt) {
            const char* buf = smem + (kt & 1) * T256_BUF;
            // ---- phase A: quadrants (0,0) (0,1): fragments of HB0, HA0, HB1; stage HB1(kt+1), HA1(kt+1)
            read_B<0>(buf, b0);
            read_A<0, 4>(buf, a);
            read_B<1>(buf, b1);
            stage_B<1>(kt + 1);
            stage_A<1>(kt + 1);
            wait_all_but<4>();                                  // HA1(kt) landed (younger: HA0 HB0 HB1 HA1 of kt+1)
            __builtin_amdgcn_sched_barrier(0);
            mfma_section2<0, 0, 1>(acc, a, b0, b1);
            // ---- phase B: quadrants (1,1) (1,0): fragments of HA1; stage HA0(kt+2), HB0(kt+2)
            read_A<1, NMT - 4>(buf, a);
            stage_A<0>(kt + 2);
            stage_B<0>(kt + 2);
            wait_all_but<3>();                                  // HB1(kt+1) (and the older HA0 / HB0(kt+1)) landed (younger: HA1(kt+1) HA0 HB0(kt+2))
            __builtin_amdgcn_sched_barrier(0);
            mfma_section2<1, 1, 0>(acc, a, b1, b0);
        }
        close();
    }
};
