// trace_device.h -- device functions of the hot path (gfx950), one header per layer; each includes the one below it.
//
//   trace_math.h            V3, Basis, Ray, RayState, compare-selects, pick / permuted
//   trace_geometry.h        camera sample            reference src/Terra.c:1783-1799
//                           slab test                reference src/Terra.c:851-878
//                           watertight ray/triangle  reference src/TerraGeometry.c:98-138, 159-260
//                           Moeller-Trumbore         reference src/Terra.c:880-922 (unit level only)
//   traverse_ref.h          BVH stack traversal      reference src/TerraBVH.c:250-310
//   traverse_fast.h         the fast tree's traversal (DESIGN.md "Fast tree")
//   shading_device.h        raycast + surface init   reference src/Terra.c:1623-1657, 1726-1764, TerraMath.inl:251-272
//                           diffuse / Phong presets  reference src/TerraPresets.c:34-146
//   integrators_device.h    integrators              reference src/Terra.c:1099-1587
//                           bounce loop              reference src/Terra.c:1039-1097
//                           tonemap                  reference src/Terra.c:578-627, 1815-1828
//
// Arithmetic rules (DESIGN.md "Bit-faithful arithmetic"): binary32 everywhere the
// reference is binary32, the reference's double promotions kept, operation order
// kept, no FMA contraction (-ffp-contract=off), IEEE division and square root,
// compare-select min/max where a NaN could reach them.
#pragma once
#include "trace_math.h"
#include "trace_geometry.h"
#include "traverse_ref.h"
#include "traverse_fast.h"
#include "shading_device.h"
#include "integrators_device.h"
