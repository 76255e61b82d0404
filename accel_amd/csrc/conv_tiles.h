// The launch geometries of the convolution kernels: one row per id (`tile=` of a plan, ConvParams::force_tile, the tile column of
// the tune tables), stated once.  conv_tiles.cpp turns the lists below into the descriptors; conv_igemm.hip expands the igemm lists
// a second time into its template switch, so the shape of an id is written in one place.  Host only.
#pragma once

enum ConvFamily {
    CONV_FAM_IGEMM, CONV_FAM_IGEMM_PIPE, CONV_FAM_IGEMM_DEEP,   // conv_igemm.hip, fp32 MFMA: plain / software-pipelined (MID 2) / deep-prefetch (MID 3) schedule
    CONV_FAM_IGEMM_DMA,                                         // ... operands by LDS-DMA
    CONV_FAM_B3,                                                // conv_igemm.hip bf16x3 kernel of an fp32 layer
    CONV_FAM_B3R,                                               // conv_b3r.hip: bf16x3 / fp16x2 of an fp32 layer, fp16 of an f16-mode layer
    CONV_FAM_B3D,                                               // conv_b3d.hip: f16-mode layers only, fp32 or half views
    CONV_FAM_WINO, CONV_FAM_WINO_B3, CONV_FAM_WINO_B3U, CONV_FAM_WINO_B3S,   // conv_wino.hip, conv_wino_b3.hip (linear / union loader), conv_wino_b3s.hip
    CONV_FAM_STEM, CONV_FAM_STEM_B3, CONV_FAM_WS, CONV_FAM_HALO,
    CONV_FAM_DIAG_IGEMM, CONV_FAM_DIAG_B3R                      // timing-only ablations (they compute wrong results): diagnostics build
};
// the weight copy of ConvParams a family reads (finalize_conv makes a copy for the layers that can take its family, or when the id is forced)
enum ConvWeights { CONV_W, CONV_W_WB3, CONV_W_WB3R, CONV_W_WH2R, CONV_W_WU, CONV_W_WUB, CONV_W_WSTEM, CONV_W_WSTEMB, CONV_W_WWS };
enum {
    CONV_T_DIAG = 1,      // exists under ACCEL_CONV_DIAG only
    CONV_T_TUNE = 2,      // conv_candidates takes it from the table (to the layers its family takes; 40, 50, 51, 60 and 78 it offers by name)
    CONV_T_F16 = 4,       // ... also to f16- and bf16x3-mode layers: the id whose own shape is the one such a layer runs on (shape16)
    CONV_T_NOSPLIT = 8,   // the family never splits K
    CONV_T_OVER64 = 16,   // offered to layers with more than 64 output channels only (conv_b3d.hip: every tile but the 64-column one)
    CONV_T_OVER128 = 32,  // ... with more than 128 only (its 256-column tiles)
};

struct ConvTile {
    int id, family;
    int bm, bn, bk;       // nominal block, pixels x output channels x K per step: what conv_plan_split counts blocks and steps in
                          // (Winograd: 64 tiles of 2x2 pixels, steps of 8 or 16 input channels)
    int weights;          // ConvWeights
    int shape16;          // row of CONV_SHAPES16 an f16- or bf16x3-mode layer runs this id on (igemm families), the family's own (b3)
    unsigned flags;
};
const ConvTile* conv_tile_row(int id);   // the row whatever the build; nullptr: no such id
const ConvTile* conv_tile(int id);       // nullptr: not part of this build
const ConvTile& conv_tile_planned(int id);   // the row conv_plan_split plans with: the id's, or 64x64x32 for an id without a row (quirks, below)
// what conv_pick_tile gives a layer with half views (conv_b3d.hip alone reads and writes them): up to 64 output channels / more
#define CONV_TILE_HALF_NARROW 88
#define CONV_TILE_HALF 84
#define CONV_TILE_IDS 100                // ids are 0 .. 99

// Quirks, kept as they are (tests/golden/conv_geometry.json pins them):
//  * an f16- or bf16x3-mode layer forced to an igemm id runs launch_f16 / launch_b3 on the id's shape16 -- 0 / 5, 1 / 6, 2 / 7 and 10 on
//    their own shape, every other id (the narrow-N ones, the 8-wavefront 11 / 12, BK 64 / 16, DMA, deep-prefetch; also 70-81 where the
//    family does not take the mode) on 64x64 -- while conv_plan_split counts blocks in the id's nominal bm x bn;
//  * an id without a row is planned as 64x64x32 (ACCEL_WB3_FORCE can name one; its launch is refused);
//  * 86 / 87 are rows (valid ids, planned as 256x256 / 128x256) that launch_conv_b3d refuses: retired shapes of conv_b3d.hip.

// shapes of the two 16-bit kernels of conv_igemm.hip (launch_f16, launch_b3): row, BM, BN, WGM, WGN; launch_b3 has 256x128 / 4x2 (row 5) besides
#define CONV_SHAPES16(X) X(0, 128, 128, 2, 2) X(1, 128, 64, 2, 2) X(2, 64, 128, 2, 2) X(3, 64, 64, 2, 2) X(4, 128, 128, 2, 4)

// conv_igemm_f32_kernel: id, BM, BN, WGM, WGN, BK, MID, shape16, flags
#define CONV_IGEMM_TILES(X) \
    X(0, 128, 128, 2, 2, 32, 0, 0, CONV_T_TUNE | CONV_T_F16) \
    X(1, 128, 64, 2, 2, 32, 0, 1, CONV_T_TUNE | CONV_T_F16) \
    X(2, 64, 128, 2, 2, 32, 0, 2, CONV_T_TUNE | CONV_T_F16) \
    X(3, 64, 64, 2, 2, 32, 0, 3, CONV_T_TUNE | CONV_T_F16) \
    X(4, 128, 32, 4, 1, 32, 0, 3, 0) \
    X(5, 128, 128, 2, 2, 32, 2, 0, CONV_T_TUNE) \
    X(6, 128, 64, 2, 2, 32, 2, 1, CONV_T_TUNE) \
    X(7, 64, 128, 2, 2, 32, 2, 2, CONV_T_TUNE) \
    X(8, 64, 64, 2, 2, 32, 2, 3, CONV_T_TUNE) \
    X(9, 128, 32, 4, 1, 32, 2, 3, 0) \
    X(10, 128, 128, 2, 4, 32, 2, 4, CONV_T_TUNE | CONV_T_F16)   /* 8 waves, wave tile 64x32 */ \
    X(11, 128, 64, 4, 2, 32, 2, 3, CONV_T_TUNE)                 /* 8 waves, wave tile 32x32 */ \
    X(12, 64, 128, 2, 4, 32, 2, 3, CONV_T_TUNE)                 /* 8 waves, wave tile 32x32 */ \
    X(13, 64, 64, 2, 2, 64, 2, 3, CONV_T_TUNE)                  /* BK 64 */ \
    X(14, 256, 128, 4, 2, 32, 2, 3, 0)                          /* 8 waves, wave tile 64x64 (110 KB LDS, 1 block/CU) */ \
    X(15, 128, 128, 2, 2, 16, 0, 3, 0)                          /* BK 16: half the LDS, 4 blocks/CU */ \
    X(31, 64, 64, 2, 2, 32, 3, 3, CONV_T_TUNE) \
    X(32, 128, 128, 2, 4, 32, 3, 3, CONV_T_TUNE) \
    X(33, 64, 128, 2, 4, 32, 3, 3, CONV_T_TUNE) \
    X(34, 128, 64, 4, 2, 32, 3, 3, CONV_T_TUNE) \
    X(35, 128, 32, 4, 1, 32, 3, 3, CONV_T_TUNE)
// ... its ablations: id, BM, BN, WGM, WGN, ABL (1 no loads, 2 no barrier (racy), 3 both, 4 loads but no LDS stores, 8 LDS stores but no loads, 16 setprio)
#define CONV_IGEMM_DIAG_TILES(X) \
    X(20, 128, 128, 2, 2, 1) X(21, 128, 128, 2, 2, 3) X(22, 128, 128, 2, 2, 2) X(23, 64, 64, 2, 2, 3) X(24, 128, 128, 2, 2, 4) X(25, 128, 128, 2, 2, 8) \
    X(26, 64, 64, 2, 2, 4) X(27, 64, 64, 2, 2, 8) X(28, 64, 64, 2, 2, 1) X(29, 128, 128, 2, 2, 16) X(30, 64, 64, 2, 2, 16)
// conv_igemm_dma_kernel: id, BM, BN, WGM, WGN, stages of the ring (96 / 48 / 64 / 64 KB)
#define CONV_DMA_TILES(X) X(16, 128, 128, 2, 4, 3) X(17, 64, 64, 2, 2, 3) X(18, 128, 128, 2, 2, 2) X(19, 64, 64, 2, 2, 4)
// every other family (the launchers of conv_b3r.hip and conv_b3d.hip switch over their own ids): id, family, bm, bn, bk, weights, shape16, flags
#define CONV_FAMILY_TILES(X) \
    X(40, CONV_FAM_WINO, 256, 64, 8, CONV_W_WU, 3, 0) \
    X(41, CONV_FAM_WINO_B3, 256, 64, 16, CONV_W_WUB, 3, CONV_T_TUNE) \
    X(42, CONV_FAM_WINO_B3U, 256, 64, 16, CONV_W_WUB, 3, CONV_T_TUNE) \
    X(43, CONV_FAM_WINO_B3S, 256, 64, 16, CONV_W_WUB, 3, CONV_T_TUNE) \
    X(50, CONV_FAM_STEM, 64, 64, 32, CONV_W_WSTEM, 3, CONV_T_NOSPLIT) \
    X(51, CONV_FAM_STEM_B3, 64, 64, 32, CONV_W_WSTEMB, 3, CONV_T_NOSPLIT) \
    X(60, CONV_FAM_WS, 64, 64, 32, CONV_W_WWS, 3, CONV_T_NOSPLIT) \
    X(70, CONV_FAM_B3, 128, 128, 32, CONV_W_WB3, 0, CONV_T_TUNE) \
    X(71, CONV_FAM_B3, 128, 64, 32, CONV_W_WB3, 1, CONV_T_TUNE) \
    X(72, CONV_FAM_B3, 64, 128, 32, CONV_W_WB3, 2, CONV_T_TUNE) \
    X(73, CONV_FAM_B3, 64, 64, 32, CONV_W_WB3, 3, CONV_T_TUNE) \
    X(74, CONV_FAM_B3, 128, 128, 32, CONV_W_WB3, 4, CONV_T_TUNE) \
    X(75, CONV_FAM_B3, 256, 128, 32, CONV_W_WB3, 5, CONV_T_TUNE)      /* 92 KB of LDS: one block per CU, 1.5x the flops per byte fetched */ \
    X(76, CONV_FAM_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_TUNE)    /* 2x4 wavefronts */ \
    X(77, CONV_FAM_B3R, 128, 64, 32, CONV_W_WB3R, 3, CONV_T_TUNE)     /* 2x2 */ \
    X(78, CONV_FAM_HALO, 128, 128, 32, CONV_W_WH2R, 3, CONV_T_NOSPLIT)   /* fp16x2 form only */ \
    X(79, CONV_FAM_B3R, 128, 256, 32, CONV_W_WB3R, 3, CONV_T_TUNE)    /* 2x4 */ \
    X(80, CONV_FAM_B3R, 128, 256, 32, CONV_W_WB3R, 3, CONV_T_TUNE)    /* 1x8 */ \
    X(81, CONV_FAM_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_TUNE)    /* 1x4 */ \
    X(82, CONV_FAM_B3D, 256, 256, 32, CONV_W_WB3R, 3, CONV_T_TUNE | CONV_T_OVER64 | CONV_T_OVER128)    /* 4x2 */ \
    X(83, CONV_FAM_B3D, 128, 256, 32, CONV_W_WB3R, 3, CONV_T_TUNE | CONV_T_OVER64 | CONV_T_OVER128)    /* 4x2 */ \
    X(84, CONV_FAM_B3D, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_TUNE | CONV_T_OVER64)    /* 4x1 */ \
    X(85, CONV_FAM_B3D, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_TUNE | CONV_T_OVER64)    /* 2x2 */ \
    X(86, CONV_FAM_B3D, 256, 256, 32, CONV_W_WB3R, 3, 0)              /* retired */ \
    X(87, CONV_FAM_B3D, 128, 256, 32, CONV_W_WB3R, 3, 0)              /* retired */ \
    X(88, CONV_FAM_B3D, 128, 64, 32, CONV_W_WB3R, 3, CONV_T_TUNE)     /* 4x1 */ \
    X(89, CONV_FAM_B3D, 256, 128, 32, CONV_W_WB3R, 3, CONV_T_TUNE | CONV_T_OVER64)    /* 4x2 */ \
    X(90, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG) \
    X(91, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG) \
    X(92, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG) \
    X(93, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG) \
    X(94, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG) \
    X(95, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG) \
    X(96, CONV_FAM_DIAG_B3R, 128, 128, 32, CONV_W_WB3R, 3, CONV_T_DIAG)
