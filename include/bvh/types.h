/* types.h — POD layouts of the BVH build path.  Binary-compatible with the reference's src/Common.h:
 *   Aabb      24 B  (src/Common.h:310-416)      Triangle  64 B, alignas(64), 36-B payload (src/Common.h:429-434)
 *   Bvh2Node  32 B, alignas(32) (src/Common.h:436-441)      PrimRef   28 B (src/Common.h:574-578)
 *   Ray       32 B, alignas(32) (src/Common.h:533-539; the record bvh_generate_rays writes)      bvh_hit 16 B (bvh_intersect's output, no counterpart)
 *   bvh_instance 64 B (one placed bottom-level tree of a bvh_scene)      bvh_instance_hit 32 B (bvh_scene_intersect's output); neither has a counterpart
 *   bvh_point_query 16 B (bvh_closest_point's input)      bvh_point_hit 32 B (its output); neither has a counterpart
 *   bvh_instance_point_hit 32 B (bvh_scene_closest_point's output: bvh_point_hit with the instance in its last word); no counterpart
 *   bvh_winding_moment 32 B (one internal node's record of bvh_winding_prepare, read by bvh_winding_number); no counterpart
 *   bvh_winding_map 64 B (one instance's record of bvh_scene_winding_prepare: cofactor matrix and scale bound); no counterpart
 *   bvh_knn_hit 8 B (one entry of bvh_knn's lists and one record of bvh_radius_search's slices; both read bvh_point_query too); no counterpart
 *   bvh_tri_hit 16 B (bvh_closest_tris's output: the nearest tree triangle to a query triangle); no counterpart
 *   bvh_instance_knn_hit 16 B (one entry of bvh_scene_knn's lists and one record of bvh_scene_radius_search's slices: bvh_knn_hit with the instance, padded to one
 *     16-byte store); no counterpart
 *   bvh_instance_tri_hit 16 B (bvh_scene_closest_tris's output and one record of bvh_scene_radius_tris's slices: bvh_tri_hit with the instance in its last
 *     word); no counterpart
 *   bvh_instance_prim 8 B (one record of bvh_scene_overlap's, bvh_scene_intersect_tris's and bvh_scene_collide's slices: a primitive of an instance); no counterpart
 * Usable from C, C++ and HIP device code. */
#ifndef BVH_TYPES_H
#define BVH_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
#define BVH_ALIGNAS(n) alignas(n)
#else
#define BVH_ALIGNAS(n) _Alignas(n)
#endif

#define BVH_INVALID 0xFFFFFFFFu                 /* INVALID_NODE_IDX / INVALID_PRIM_IDX, src/Common.h:90-92 */
#define BVH_FLT_MAX 3.402823466e+38f            /* FltMax, src/Common.h:86 */

typedef struct { float x, y, z; } bvh_float3;
typedef struct { bvh_float3 min, max; } bvh_aabb;
typedef struct BVH_ALIGNAS(64) { bvh_float3 v1, v2, v3; } bvh_triangle;
typedef struct BVH_ALIGNAS(32) { uint32_t left, right; bvh_aabb aabb; } bvh2_node;
typedef struct { uint32_t prim_idx; bvh_aabb aabb; } bvh_primref;
typedef struct BVH_ALIGNAS(32) { bvh_float3 origin, direction; float tmin, tmax; } bvh_ray;
typedef struct { float t, u, v; uint32_t prim_idx; } bvh_hit;
/* point: the query point; radius: the search radius (+inf: unbounded).  Hit: point = the closest point of triangle prim_idx, dist2 = its squared distance,
 * (u, v) = the weights of v2 and v3 */
typedef struct { bvh_float3 point; float radius; } bvh_point_query;
typedef struct { bvh_float3 point; float dist2; float u, v; uint32_t prim_idx, reserved; } bvh_point_hit;
/* bvh_winding_prepare's record of one internal node: (ax, ay, az) = the sum of its triangles' area vectors, area = the sum of their areas, (px, py, pz) = their
 * area-weighted centroid (the centre of the node's box when area is 0 or non-finite), r = the distance from p to the farthest corner of the node's box */
typedef struct { float ax, ay, az, area; float px, py, pz, r; } bvh_winding_moment;
/* bvh_scene_winding_prepare's record of one instance with object_to_world [A | t]: c = the cofactor matrix of A, row-major (it maps area vectors:
 * cross(A u, A v) = C (u x v)), smax = a bound on A's largest singular value; all zero for an inactive instance */
typedef struct { float c[9]; float smax; uint32_t reserved[6]; } bvh_winding_map;
/* one entry of a k-nearest list (bvh_knn) or of a radius search's slice (bvh_radius_search): the squared distance of triangle prim_idx's closest point (an
 * unused slot of a k-nearest list: {radius*radius, BVH_INVALID}; a slice has no unused slots) */
typedef struct { float dist2; uint32_t prim_idx; } bvh_knn_hit;
/* bvh_closest_tris's answer to one query triangle: dist2 = the squared distance to tree triangle prim_idx, feature = which of the 16 terms of the header's
 * dist2(X, Y) gave it (0..2: a query vertex against the tree triangle, 3..5: a tree vertex against the query triangle, 6 + 3*i + j: edge i of the query against
 * edge j of the tree triangle, 15: a proper crossing); a miss: {radius*radius, BVH_INVALID, 0, 0} */
typedef struct { float dist2; uint32_t prim_idx; uint32_t feature; uint32_t reserved; } bvh_tri_hit;
/* object_to_world: row-major 3x4 matrix {m00 m01 m02 m03, m10 .. m13, m20 .. m23}; world = M * (object, 1).  blas: index into the scene's bottom-level table */
typedef struct { float object_to_world[12]; uint32_t blas; uint32_t reserved[3]; } bvh_instance;
typedef struct { float t, u, v; uint32_t prim_idx, instance_idx; uint32_t reserved[3]; } bvh_instance_hit;
/* point: the closest point of instance instance_idx's triangle prim_idx in WORLD space, dist2 = its squared world distance, (u, v) = the weights of v2 and v3 */
typedef struct { bvh_float3 point; float dist2; float u, v; uint32_t prim_idx, instance_idx; } bvh_instance_point_hit;
/* one entry of a scene's k-nearest list (bvh_scene_knn) and one record of bvh_scene_radius_search's slices: the squared WORLD distance of instance
 * instance_idx's triangle prim_idx; reserved = 0 (an unused slot of a k-nearest list: {radius*radius, BVH_INVALID, BVH_INVALID, 0}; a slice has no unused slots) */
typedef struct { float dist2; uint32_t prim_idx, instance_idx, reserved; } bvh_instance_knn_hit;
/* bvh_scene_closest_tris's answer to one query triangle: dist2 = the squared WORLD distance to triangle prim_idx of instance instance_idx, feature as in
 * bvh_tri_hit; a miss: {radius*radius, BVH_INVALID, 0, BVH_INVALID}.  Also one record of bvh_scene_radius_tris's slices (a slice has no miss records) */
typedef struct { float dist2; uint32_t prim_idx; uint32_t feature; uint32_t instance_idx; } bvh_instance_tri_hit;
/* one record of bvh_scene_overlap's, bvh_scene_intersect_tris's and bvh_scene_collide's slices: triangle prim_idx of instance instance_idx (a slice has no unused slots) */
typedef struct { uint32_t prim_idx, instance_idx; } bvh_instance_prim;

#ifdef __cplusplus
static_assert(sizeof(bvh_aabb) == 24, "Aabb is 24 bytes");
static_assert(sizeof(bvh_triangle) == 64, "Triangle is 64 bytes");
static_assert(sizeof(bvh2_node) == 32, "Bvh2Node is 32 bytes");
static_assert(sizeof(bvh_primref) == 28, "PrimRef is 28 bytes");
static_assert(sizeof(bvh_ray) == 32, "Ray is 32 bytes");
static_assert(sizeof(bvh_hit) == 16, "bvh_hit is 16 bytes");
static_assert(sizeof(bvh_point_query) == 16, "bvh_point_query is 16 bytes");
static_assert(sizeof(bvh_point_hit) == 32, "bvh_point_hit is 32 bytes");
static_assert(sizeof(bvh_winding_moment) == 32, "bvh_winding_moment is 32 bytes");
static_assert(sizeof(bvh_winding_map) == 64, "bvh_winding_map is 64 bytes");
static_assert(sizeof(bvh_knn_hit) == 8, "bvh_knn_hit is 8 bytes");
static_assert(sizeof(bvh_tri_hit) == 16, "bvh_tri_hit is 16 bytes");
static_assert(sizeof(bvh_instance) == 64, "bvh_instance is 64 bytes");
static_assert(sizeof(bvh_instance_hit) == 32, "bvh_instance_hit is 32 bytes");
static_assert(sizeof(bvh_instance_point_hit) == 32, "bvh_instance_point_hit is 32 bytes");
static_assert(sizeof(bvh_instance_knn_hit) == 16, "bvh_instance_knn_hit is 16 bytes");
static_assert(sizeof(bvh_instance_tri_hit) == 16, "bvh_instance_tri_hit is 16 bytes");
static_assert(sizeof(bvh_instance_prim) == 8, "bvh_instance_prim is 8 bytes");
#endif

#endif
