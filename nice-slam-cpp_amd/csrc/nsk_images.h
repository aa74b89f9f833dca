// nsk_images.h -- the derived copies ("images") of a decoder's parameters that the MFMA kernels read: what each one is (ImageSpec) and the index
// table that builds it, in host integers, nothing of HIP (host/test/images_test.cpp builds it with a plain host compiler:
// tests/test_images_cpu.py; nsk_decoder_image_table of include/nsk.h hands the tables out without a device)
//
// what = 0 the fp32 forward image (MlpFwdImg / CoarseFwdImg), 1 the fp32 backward image (MlpBwdImg / CoarseBwdImg), 2 the forward image in
// 16-bit pieces (MlpFwdImgB) + fp32 tail, 3 the backward image in fp16 pieces (MlpBwdImgH) + fp32 tail; the coarse decoder has only 0 and 1.
// A table entry is the canonical (nsk_dec_layout) offset of the parameter that image position holds, or -1 for a position that stays zero.
// The tables of images 2 and 3 cover the fragments only: their fp32 tail is a copy of the last tail_n floats of the fp32 sibling (what - 2).
// The backward images of the fine decoder (c_dim 64) cover only the first 32 feature columns of fc[l] (seg_bwd / build_idx16b with
// ld = c_dim and 32 rows): the other 32 columns are in no backward image, which is why `set` is smaller there than in the forward images.
#pragma once
#include <cstddef>
#include <vector>
#include "nsk_layout.h"

#define NSK_NUM_IMAGES 4

struct ImageSpec {
    int floats = 0;        // size of the image, fragments and tail (0: the decoder has no such image)
    int entries = 0;       // entries of its index table
    int pieces = 0;        // 16-bit pieces per weight: 0 = plain fp32, 2 = fp16 high + 2048-fold low, 3 = bf16
    int tail_off = 0;      // float offset of its fp32 tail
    int sib_off = 0;       // the tail mirrors the fp32 sibling's table from this entry on
    int tail_n = 0;        // floats of the tail (0: none)
};

// an image in pieces: entries x pieces unsigned shorts, then the tail
inline ImageSpec with_pieces(ImageSpec s, int pieces)
{
    s.pieces = pieces; s.tail_off = s.entries * pieces / 2; s.floats = s.tail_off + s.tail_n;
    return s;
}

// the tails: biases, Wo, bo, B of the forward image (740 floats); Wo, B of the backward image (416)
template <int CQ> struct FwdTail {
    static constexpr int N = MlpFwdImg<CQ>::TOTAL - MlpFwdImg<CQ>::P_B;
    static_assert(MlpFwdImgB<CQ, 2>::TOTAL_F - MlpFwdImgB<CQ, 2>::P_F32 == N && MlpFwdImgB<CQ, 3>::TOTAL_F - MlpFwdImgB<CQ, 3>::P_F32 == N,
                  "the forward image in pieces ends in the tail of the fp32 forward image");
    static_assert(MlpFwdImgB<CQ, 2>::P_F32 == MlpFwdImgB<CQ, 2>::NBLK * 1024 && 2 * MlpFwdImgB<CQ, 3>::P_F32 == 3 * MlpFwdImgB<CQ, 3>::NBLK * 1024,
                  "with_pieces places the tail where MlpFwdImgB does");
};
static constexpr int BWD_TAIL_N = MlpBwdImg::TOTAL - MlpBwdImg::P_WO;
static_assert(MlpBwdImgH::TOTAL_F - MlpBwdImgH::P_WO == BWD_TAIL_N && MlpBwdImgH::P_WO == MlpBwdImgH::NFG * 512,
              "the fp16 backward image ends in the tail of the fp32 backward image, where with_pieces places it");
static_assert(FwdTail<2>::N == 740 && FwdTail<4>::N == 740 && BWD_TAIL_N == 416, "tail sizes");

// image `what` of decoder `which`; pieces (2 or 3) counts for image 2 alone -- image 3 is always two fp16 pieces
inline ImageSpec image_spec(int which, int what, int pieces)
{
    ImageSpec s;
    const bool fine = which == 2;
    if (what == 0) s.floats = s.entries = which == 0 ? CoarseFwdImg::TOTAL : (fine ? MlpFwdImg<4>::TOTAL : MlpFwdImg<2>::TOTAL);
    if (what == 1) s.floats = s.entries = which == 0 ? CoarseBwdImg::TOTAL : MlpBwdImg::TOTAL;
    if (what < 2 || which == 0) return s;
    if (what == 2) {
        s.entries = (fine ? MlpFwdImgB<4>::NBLK : MlpFwdImgB<2>::NBLK) * 2 * 512;
        s.sib_off = fine ? MlpFwdImg<4>::P_B : MlpFwdImg<2>::P_B; s.tail_n = FwdTail<2>::N;
        return with_pieces(s, pieces);
    }
    s.entries = MlpBwdImgH::NFG * 512;
    s.sib_off = MlpBwdImg::P_WO; s.tail_n = BWD_TAIL_N;
    return with_pieces(s, 2);
}

// ---- the index tables -----------------------------------------------------------------------------------
static void seg_fwd(std::vector<int>& idx, int quad0, int KQ, int Wofs, int ld, int col0, int kvalid)
{
    for (int rt = 0; rt < 2; ++rt) for (int q = 0; q < KQ; ++q) for (int lane = 0; lane < 64; ++lane) for (int i = 0; i < 4; ++i) {
        int o = 16 * rt + (lane & 15), k = 16 * q + 4 * (lane >> 4) + i;
        idx[((size_t)(quad0 + rt * KQ + q) * 64 + lane) * 4 + i] = k < kvalid ? Wofs + o * ld + col0 + k : -1;
    }
}
static void seg_bwd(std::vector<int>& idx, int quad0, int RT, int Wofs, int ld, int col0, int rvalid)
{
    const int KQ = 2;
    for (int rt = 0; rt < RT; ++rt) for (int q = 0; q < KQ; ++q) for (int lane = 0; lane < 64; ++lane) for (int i = 0; i < 4; ++i) {
        int r = 16 * rt + (lane & 15), k = 16 * q + 4 * (lane >> 4) + i;
        idx[((size_t)(quad0 + rt * KQ + q) * 64 + lane) * 4 + i] = r < rvalid ? Wofs + k * ld + col0 + r : -1;
    }
}

template <int CQ>
static void build_mlp_fwd_idx(const DecLayout& L, std::vector<int>& idx)
{
    typedef MlpFwdImg<CQ> I;
    idx.assign(I::TOTAL, -1);
    seg_fwd(idx, I::W0E, 6, L.oW[0], NSK_E, 0, NSK_E);
    for (int l = 0; l < 5; ++l) seg_fwd(idx, I::F(l), CQ, L.oFw[l], L.c_dim, 0, L.c_dim);
    seg_fwd(idx, I::W1, 2, L.oW[1], 32, 0, 32);
    seg_fwd(idx, I::W2, 2, L.oW[2], 32, 0, 32);
    seg_fwd(idx, I::W3E, 6, L.oW[3], 125, 0, NSK_E);
    seg_fwd(idx, I::W3H, 2, L.oW[3], 125, NSK_E, 32);
    seg_fwd(idx, I::W4, 2, L.oW[4], 32, 0, 32);
    for (int l = 0; l < 5; ++l) for (int o = 0; o < 32; ++o) { idx[I::P_B + 32 * l + o] = L.ob[l] + o; idx[I::P_BC + 32 * l + o] = L.oFb[l] + o; }
    for (int o = 0; o < L.out_dim; ++o) { for (int k = 0; k < 32; ++k) idx[I::P_WO + 32 * o + k] = L.oWo + 32 * o + k; idx[I::P_BO + o] = L.obo + o; }
    for (int a = 0; a < 3; ++a) for (int k = 0; k < NSK_E; ++k) idx[I::P_BM + 96 * a + k] = L.oB + NSK_E * a + k;
}

static void build_idx(int w, std::vector<int>& fidx, std::vector<int>& bidx)
{
    DecLayout L = nsk_dec_layout(w);
    if (w == 0) {
        typedef CoarseFwdImg I; typedef CoarseBwdImg J;
        fidx.assign(I::TOTAL, -1); bidx.assign(J::TOTAL, -1);
        seg_fwd(fidx, I::W0, 2, L.oW[0], 32, 0, 32); seg_fwd(fidx, I::W1, 2, L.oW[1], 32, 0, 32); seg_fwd(fidx, I::W2, 2, L.oW[2], 32, 0, 32);
        seg_fwd(fidx, I::W3C, 2, L.oW[3], 64, 0, 32); seg_fwd(fidx, I::W3H, 2, L.oW[3], 64, 32, 32); seg_fwd(fidx, I::W4, 2, L.oW[4], 32, 0, 32);
        for (int l = 0; l < 5; ++l) for (int o = 0; o < 32; ++o) fidx[I::P_B + 32 * l + o] = L.ob[l] + o;
        for (int k = 0; k < 32; ++k) fidx[I::P_WO + k] = L.oWo + k;
        fidx[I::P_BO] = L.obo;
        seg_bwd(bidx, J::W0T, 2, L.oW[0], 32, 0, 32); seg_bwd(bidx, J::W1T, 2, L.oW[1], 32, 0, 32); seg_bwd(bidx, J::W2T, 2, L.oW[2], 32, 0, 32);
        seg_bwd(bidx, J::W3CT, 2, L.oW[3], 64, 0, 32); seg_bwd(bidx, J::W3HT, 2, L.oW[3], 64, 32, 32); seg_bwd(bidx, J::W4T, 2, L.oW[4], 32, 0, 32);
        for (int k = 0; k < 32; ++k) bidx[J::P_WO + k] = L.oWo + k;
        return;
    }
    if (w == 2) build_mlp_fwd_idx<4>(L, fidx); else build_mlp_fwd_idx<2>(L, fidx);
    typedef MlpBwdImg J;
    bidx.assign(J::TOTAL, -1);
    for (int l = 0; l < 5; ++l) seg_bwd(bidx, J::FT(l), 2, L.oFw[l], L.c_dim, 0, 32);
    for (int l = 1; l < 5; ++l) seg_bwd(bidx, J::WT(l), 2, L.oW[l], L.in_dim[l], l == 3 ? NSK_E : 0, 32);
    seg_bwd(bidx, J::W0ET, 6, L.oW[0], NSK_E, 0, NSK_E);
    seg_bwd(bidx, J::W3ET, 6, L.oW[3], 125, 0, NSK_E);
    for (int o = 0; o < L.out_dim; ++o) for (int k = 0; k < 32; ++k) bidx[J::P_WO + 32 * o + k] = L.oWo + 32 * o + k;
    for (int a = 0; a < 3; ++a) for (int k = 0; k < NSK_E; ++k) bidx[J::P_BM + 96 * a + k] = L.oB + NSK_E * a + k;
}

static void seg16(std::vector<int>& idx, int blk0, int NB, int Wofs, int ld, int col0, int kvalid)
{
    for (int b = 0; b < NB; ++b) for (int rt = 0; rt < 2; ++rt) for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 8; ++j) {
        int fg = 2 * (blk0 + b) + rt, o = 16 * rt + (lane & 15), k = 32 * b + nsk_bf16_kperm(lane >> 4, j);
        idx[((size_t)fg * 64 + lane) * 8 + j] = k < kvalid ? Wofs + o * ld + col0 + k : -1;
    }
}
template <int CQ>
static void build_idx16(const DecLayout& L, std::vector<int>& idx)
{
    typedef MlpFwdImgB<CQ> I;
    idx.assign((size_t)I::NBLK * 2 * 512, -1);
    seg16(idx, I::W0E, 3, L.oW[0], NSK_E, 0, NSK_E);
    for (int l = 0; l < 5; ++l) seg16(idx, I::F(l), I::CB, L.oFw[l], L.c_dim, 0, L.c_dim);
    seg16(idx, I::W1, 1, L.oW[1], 32, 0, 32); seg16(idx, I::W2, 1, L.oW[2], 32, 0, 32); seg16(idx, I::W4, 1, L.oW[4], 32, 0, 32);
    seg16(idx, I::W3E, 3, L.oW[3], 125, 0, NSK_E); seg16(idx, I::W3H, 1, L.oW[3], 125, NSK_E, 32);
}

static void build_idx16b(const DecLayout& L, std::vector<int>& idx)
{
    typedef MlpBwdImgH J;
    idx.assign((size_t)J::NFG * 512, -1);
    auto seg = [&](int fg0, int nrt, int Wofs, int ld, int col0, int rows) {   // transposed: row o = input column, k = output row of the forward weight
        for (int rt = 0; rt < nrt; ++rt) for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 8; ++j) {
            const int o = 16 * rt + (lane & 15), k = nsk_bf16_kperm(lane >> 4, j);
            idx[((size_t)(fg0 + rt) * 64 + lane) * 8 + j] = o < rows ? Wofs + k * ld + col0 + o : -1;
        }
    };
    for (int l = 0; l < 5; ++l) seg(J::FT(l), 2, L.oFw[l], L.c_dim, 0, 32);
    for (int l = 1; l < 5; ++l) seg(J::WT(l), 2, L.oW[l], L.in_dim[l], l == 3 ? NSK_E : 0, 32);
    seg(J::W0ET, 6, L.oW[0], NSK_E, 0, NSK_E);
    seg(J::W3ET, 6, L.oW[3], 125, 0, NSK_E);
}

// the table of image `what` of decoder `which` (image_spec's entries of them; none for an image the decoder does not have); it does not depend
// on the piece count
static void build_image_table(int which, int what, std::vector<int>& idx)
{
    std::vector<int> other;
    idx.clear();
    if (what == 0) build_idx(which, idx, other);
    else if (what == 1) build_idx(which, other, idx);
    else if (which == 0) return;
    else if (what == 3) build_idx16b(nsk_dec_layout(which), idx);
    else if (which == 2) build_idx16<4>(nsk_dec_layout(which), idx);
    else build_idx16<2>(nsk_dec_layout(which), idx);
}

// inv[k] = the entry that holds parameter k (-1 none), for k < n.  Returns -1, or the first parameter that a second entry holds (inv is then
// incomplete): the optimiser launch rewrites one image position per parameter.
static int invert_table(const std::vector<int>& idx, size_t n, std::vector<int>& inv)
{
    inv.assign(n, -1);
    for (size_t t = 0; t < idx.size(); ++t) if (idx[t] >= 0) { if (inv[idx[t]] != -1) return idx[t]; inv[idx[t]] = (int)t; }
    return -1;
}
