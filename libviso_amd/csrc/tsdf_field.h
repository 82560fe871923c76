// tsdf_field.h — what tsdf_field.hip and tsdf_travel.hip share of a distance field (include/viso_hip.h, "TSDF distance field"): the
// box as the kernels take it, the check of a caller's box, and the device part of the field into buffers that the caller owns.
#ifndef VISO_TSDF_FIELD_H_
#define VISO_TSDF_FIELD_H_
#include "tsdf_table.h"

#define FIELD_MAX_AXIS 512

struct FieldBox {
    int32_t lo[3];
    uint32_t n[3];
    uint32_t cells;   // n0 n1 n2 <= 2^27
};

// The box of a call (non-null) as a FieldBox: false, with the error text set, unless every axis has 1 .. FIELD_MAX_AXIS voxels.
// Touches no device.
bool field_box_arg(const char* where, const viso_voxel_box* box, FieldBox* b);

// The sites kernel and the three passes over the box b, on the stream of h (entered, locked and not overflowed): d_state receives
// the states, `result` the field, *n_sites the number of sites; `other` is the passes' second buffer and holds nothing of use
// afterwards.  result and other: b.cells uint32 each, d_state: b.cells bytes, all on the device.  Waits for the launches.
int field_passes(VoxelHost* h, const TsdfTable& t, uint32_t min_weight, const FieldBox& b, uint32_t unknown_is_site, uint32_t* result,
                 uint32_t* other, uint8_t* d_state, unsigned long long* n_sites);
#endif /* VISO_TSDF_FIELD_H_ */
