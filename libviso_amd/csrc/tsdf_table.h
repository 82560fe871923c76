// tsdf_table.h — what tsdf.hip and tsdf_align.hip share of a TSDF map: the table's layout on the device and, of a live handle, the
// table with the constants derived from its parameters.  The map itself (struct viso_tsdf), its registry and its kernels stay in
// tsdf.hip.
#ifndef VISO_TSDF_TABLE_H_
#define VISO_TSDF_TABLE_H_
#include "voxel_host.h"

struct TsdfTable {
    VoxelTable head;
    unsigned long long* sum; uint32_t* weight;   // [slots] i64 (added as u64, two's complement), [slots]
};

// a live map's table as a reader takes it (gray: a gray map's sums of intensities [slots], null for a plain map)
struct TsdfView {
    TsdfTable t;
    const unsigned long long* gray;
    double voxel, s;      // s = voxel / 1024
    int trunc_voxels;
};

VoxelRegistry& tsdf_registry();                 // the live TSDF maps
void tsdf_view(viso_tsdf* t, TsdfView* out);    // t is live (the registry has answered for it)
#endif /* VISO_TSDF_TABLE_H_ */
