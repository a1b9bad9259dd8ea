// tile_pass.h -- what one launch of the tile transform (tile_transform.h) does to a transform of 2^logn points.  Part of the kernel arguments of
// both encoders (CkFft, BfvNtt) and filled in by Context::tile_two_pass.
#pragma once

namespace mkhe {

struct TilePass {
    int logn, logt;         // points of the transform and of a tile
    int a_log;              // > 0: column tiles of 2^a_log rows
    int first, last;        // this launch reads the caller's input / writes the caller's output
};

}  // namespace mkhe
