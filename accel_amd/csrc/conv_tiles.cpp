// The launch-geometry descriptors (conv_tiles.h): the lists expanded into one switch, so a lookup is a jump, not a search.
#include "kernels.h"

const ConvTile* conv_tile_row(int id)
{
    switch (id) {
#define IGEMM_ROW(ID, BM, BN, WGM, WGN, BK, MID, S16, FLAGS) \
    case ID: { static const ConvTile t = {ID, MID == 3 ? CONV_FAM_IGEMM_DEEP : MID == 2 ? CONV_FAM_IGEMM_PIPE : CONV_FAM_IGEMM, BM, BN, BK, CONV_W, S16, FLAGS}; return &t; }
#define DIAG_ROW(ID, BM, BN, WGM, WGN, ABL) \
    case ID: { static const ConvTile t = {ID, CONV_FAM_DIAG_IGEMM, BM, BN, 32, CONV_W, 3, CONV_T_DIAG}; return &t; }
#define DMA_ROW(ID, BM, BN, WGM, WGN, STAGES) \
    case ID: { static const ConvTile t = {ID, CONV_FAM_IGEMM_DMA, BM, BN, 32, CONV_W, 3, 0}; return &t; }
#define FAMILY_ROW(ID, FAMILY, BM, BN, BK, WEIGHTS, S16, FLAGS) \
    case ID: { static const ConvTile t = {ID, FAMILY, BM, BN, BK, WEIGHTS, S16, FLAGS}; return &t; }
        CONV_IGEMM_TILES(IGEMM_ROW)
        CONV_IGEMM_DIAG_TILES(DIAG_ROW)
        CONV_DMA_TILES(DMA_ROW)
        CONV_FAMILY_TILES(FAMILY_ROW)
#undef IGEMM_ROW
#undef DIAG_ROW
#undef DMA_ROW
#undef FAMILY_ROW
        default: return nullptr;
    }
}

const ConvTile* conv_tile(int id)
{
    const ConvTile* t = conv_tile_row(id);
#ifndef ACCEL_CONV_DIAG
    if (t && (t->flags & CONV_T_DIAG)) return nullptr;
#endif
    return t;
}

bool conv_tile_valid(int tile) { return conv_tile(tile) != nullptr; }

const ConvTile& conv_tile_planned(int id)
{
    static const ConvTile none = {-1, CONV_FAM_IGEMM, 64, 64, 32, CONV_W, 3, 0};
    const ConvTile* t = conv_tile_row(id);
    return t ? *t : none;
}
