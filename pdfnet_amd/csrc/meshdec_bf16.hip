// The fused mesh decoder (csrc/meshdec_kernels.h) with its linear products on the bf16 MFMA: MdArith::BF16 there.  A translation unit of its own
// so that the three sets of kernels compile in parallel.  Same argument block, same tape layout as the fp32 build.
#include "meshdec_kernels.h"

PDF_API int pdf_mesh_level_fwd_bf16(const PdfMeshLevel* a, void* stream) { return mesh_level_fwd<MdArith::BF16>(a, stream); }
PDF_API int pdf_mesh_level_bwd_bf16(const PdfMeshLevel* a, void* stream, void* side_stream) { return mesh_level_bwd<MdArith::BF16>(a, stream, side_stream); }
