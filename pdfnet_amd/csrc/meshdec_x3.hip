// The fused mesh decoder (csrc/meshdec_kernels.h) with its linear products as x3 arithmetic (six bf16 MFMAs per fp32 product on operands split as
// they are fed): MdArith::X3 there.  A translation unit of its own so that the three sets of kernels compile in parallel.  Same argument block, same
// tape layout as the fp32 build.
#include "meshdec_kernels.h"

PDF_API int pdf_mesh_level_fwd_x3(const PdfMeshLevel* a, void* stream) { return mesh_level_fwd<MdArith::X3>(a, stream); }
PDF_API int pdf_mesh_level_bwd_x3(const PdfMeshLevel* a, void* stream, void* side_stream) { return mesh_level_bwd<MdArith::X3>(a, stream, side_stream); }
