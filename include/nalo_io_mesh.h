/* The mesh file of the tsdf=1 path, part of include/nalo_io.h (which includes this file; a caller includes that one). Host code only. */
#ifndef NALO_IO_MESH_H
#define NALO_IO_MESH_H
#ifdef __cplusplus
extern "C" {
#endif

/* mesh.ply -- the file a user hands to a viewer: the indexed triangle list of nalo_tsdf_mesh (include/nalo_gpu.h) as PLY `format binary_little_endian 1.0`,
 * `element vertex nv` with `property float x|y|z`, `element face nt` with `property list uchar int vertex_indices`; a face is the byte 3 and three
 * little-endian int32. The header, byte for byte:
 *   "ply\nformat binary_little_endian 1.0\nelement vertex <nv>\nproperty float x\nproperty float y\nproperty float z\nelement face <nt>\n
 *    property list uchar int vertex_indices\nend_header\n"
 * xyz: [nv][3] float, tri: [nt][3] int; either count may be 0 (its array may then be NULL). NALO_IO_ERR_ARG, and no file is touched: a NULL path, a negative
 * count, a missing array, an index outside [0, nv). NALO_IO_ERR_FILE for a path that cannot be written. */
int nalo_io_write_ply_mesh(const char* path, long long nv, const float* xyz, long long nt, const int* tri);

/* the coloured mesh of nalo_tsdf_mesh_color: the same file with `property uchar red|green|blue|alpha` behind z, so that a vertex is 12 + 4 bytes (rgba:
 * [nv][4] bytes, R, G, B, A as that call writes them); faces as above. The header, byte for byte:
 *   "ply\nformat binary_little_endian 1.0\nelement vertex <nv>\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n
 *    property uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face <nt>\nproperty list uchar int vertex_indices\nend_header\n"
 * Refusals as nalo_io_write_ply_mesh, and NALO_IO_ERR_ARG for a NULL rgba with nv > 0. */
int nalo_io_write_ply_mesh_rgba(const char* path, long long nv, const float* xyz, const unsigned char* rgba, long long nt, const int* tri);

#ifdef __cplusplus
}
#endif
#endif
