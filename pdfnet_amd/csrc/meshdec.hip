// The fused mesh decoder (csrc/meshdec_kernels.h) with its linear products on the fp32 MFMA, and what the three builds share: the tape sizes and
// the diagnostics.  Entry points: pdf_mesh_level_fwd, pdf_mesh_level_bwd.
#include "meshdec_kernels.h"

PDF_API int pdf_mesh_level_fwd(const PdfMeshLevel* a, void* stream) { return mesh_level_fwd<MdArith::F32>(a, stream); }
PDF_API int pdf_mesh_level_bwd(const PdfMeshLevel* a, void* stream, void* side_stream) { return mesh_level_bwd<MdArith::F32>(a, stream, side_stream); }

PDF_API long pdf_mesh_tape_floats(int level, int B) { return level < 0 || level > 2 || B < 1 ? 0 : tape_offsets(level, B).total(); }
PDF_API long pdf_mesh_gtape_floats(int level, int B) { return level < 0 || level > 2 || B < 1 ? 0 : gtape_offsets(level, B).total(); }
PDF_API int pdf_debug_mesh_level_size() { return (int)sizeof(PdfMeshLevel); }

// diagnostic build only: copies the stage stamps of the last fp32 launches to out[8 * 3 * 64]; returns 0 when the library was built without them
#if MD_STAMPS
PDF_API int pdf_debug_mesh_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_md_stamps), sizeof(unsigned long long) * 8 * 3 * 64) == hipSuccess ? 1 : 0;
}
#else
PDF_API int pdf_debug_mesh_stamps(unsigned long long*) { return 0; }
#endif
