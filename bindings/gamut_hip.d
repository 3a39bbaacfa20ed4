/**
 * gamut_hip.d -- D binding of include/gamut_hip.h (libgamut_hip.so), the file a Gamut maintainer adds as
 * `source/gamut/hip.d`.  The C header is the source of truth; tests/test_capi_cpu.py::test_d_binding_lists_every_export
 * checks that every function the header declares is declared here with the same return and parameter TYPES (a C -> D type map),
 * ::test_d_binding_struct_layouts that the structs declared here have the header's layout (size and every field offset).
 * (No D compiler exists in the image this was written in: the file is checked textually, not compiled; the `static assert`s
 * at the end of the extern(C) block are what a D compiler will check on the first build.)
 *
 * Linkage.  Everything inside the `extern(C)` block has C linkage -- including the function-pointer TYPES it declares.
 * The reference's own callbacks do NOT: `stream_read_jpeg` (plugins/jpeg.d:167), `stb_read`, `stb_skip`, `stb_eof`
 * (codecs/stbdec.d:143-165) and the aliases / struct members that hold them (`JpegStreamReadFunc` jpegload.d:70,
 * `stbi_io_callbacks` stbdec.d:408-419) are extern(D).  `&stream_read_jpeg` therefore does not convert to
 * `gamut_hip_jpeg_stream_read_func`, and a cast that makes it compile would call a D-ABI function with the C convention
 * (DMD and LDC pass extern(D) parameters in reverse order on x86-64): `stb_read(user, data, size)` would receive
 * `(size, data, user)`.  Two correct ways to make the swap, both shown at the end of this file:
 *   (1) mark the four reference functions `extern(C)` (a one-word change each; they keep working for stb / jpgd, whose
 *       callback types then have to be extern(C) as well), or
 *   (2) leave the reference untouched and pass the four one-line extern(C) trampolines below.
 */
module gamut.hip;

nothrow @nogc:

extern(C)
{
    enum { GAMUT_HIP_OK = 0, GAMUT_HIP_ERR_INVALID_ARG, GAMUT_HIP_ERR_UNSUPPORTED, GAMUT_HIP_ERR_OUT_OF_MEMORY,
           GAMUT_HIP_ERR_HIP, GAMUT_HIP_ERR_DECODE, GAMUT_HIP_ERR_NO_DEVICE }
    enum { GAMUT_JPGD_GRAYSCALE = 0, GAMUT_JPGD_YH1V1, GAMUT_JPGD_YH2V1, GAMUT_JPGD_YH1V2, GAMUT_JPGD_YH2V2 }
    enum { GAMUT_HIP_INFLATE_E_BLOCK_TYPE = 1, GAMUT_HIP_INFLATE_E_STORED, GAMUT_HIP_INFLATE_E_LENGTHS, GAMUT_HIP_INFLATE_E_CODE,
           GAMUT_HIP_INFLATE_E_DISTANCE, GAMUT_HIP_INFLATE_E_INPUT }
    enum { GAMUT_HIP_FORMAT_UNKNOWN = -1, GAMUT_HIP_FORMAT_JPEG = 0, GAMUT_HIP_FORMAT_PNG = 1, GAMUT_HIP_FORMAT_QOI = 2, GAMUT_HIP_FORMAT_TGA = 5, GAMUT_HIP_FORMAT_BMP = 7 }
    enum GAMUT_HIP_QOI_SLACK = 160;
    enum GAMUT_HIP_COMM_ID_BYTES = 128;

    // ---- runtime ----------------------------------------------------------------------------------------------
    const(char)* gamut_hip_version();
    int   gamut_hip_device_count();
    int   gamut_hip_init(int device);
    void  gamut_hip_shutdown();
    const(char)* gamut_hip_last_error();
    void* gamut_hip_device_malloc(size_t bytes);
    void  gamut_hip_device_free(void* p);
    void* gamut_hip_host_malloc_pinned(size_t bytes);
    void  gamut_hip_host_free_pinned(void* p);
    int   gamut_hip_memcpy_h2d(void* dst, const(void)* src, size_t bytes, void* stream);
    int   gamut_hip_memcpy_d2h(void* dst, const(void)* src, size_t bytes, void* stream);
    void* gamut_hip_stream_create();
    void  gamut_hip_stream_destroy(void* stream);
    int   gamut_hip_stream_synchronize(void* stream);

    // ---- scanline.d: PixelType is passed as int (enum PixelType has base type int, same ordinals, types.d:32-59) ------
    int gamut_hip_pixel_type_size(int type);
    int gamut_hip_scanlines_inter_type(int srcType, int dstType);
    int gamut_hip_scanlines_convert(int srcType, const(ubyte)* src, int srcPitch,
                                    int dstType, ubyte* dst, int dstPitch, int width, int height);
    int gamut_hip_scanlines_copy(int type, const(ubyte)* src, int srcPitch, ubyte* dst, int dstPitch, int width, int height);
    int gamut_hip_scanlines_convert_device(int srcType, const(void)* src, long srcPitch, long srcLayerOffset,
                                           int dstType, void* dst, long dstPitch, long dstLayerOffset,
                                           int width, int height, int layers, void* stream);
    int gamut_hip_flip_device(int type, void* data, long pitch, long layerOffset, int width, int height, int layers, int vertical, void* stream);
    int gamut_hip_flip(int type, ubyte* data, int pitch, int width, int height, int vertical);

    // ---- jpegload.d ---------------------------------------------------------------------------------------------
    struct gamut_hip_jpeg_desc  { const(short)* coeffs; const(ubyte)* max_zag; ubyte* out_; long out_pitch;
                                  int width, height, scan_type, out_comps; }
    struct gamut_hip_jpeg_frame { int width, height, comps, scan_type, mcus_per_row, mcus_per_col, blocks_per_mcu;
                                  short* coeffs; ubyte* max_zag; float pixel_aspect_ratio, dpi_y; }
    int  gamut_hip_jpeg_reconstruct_device(const(gamut_hip_jpeg_desc)* descs, int count, void* stream);
    int  gamut_hip_jpeg_reconstruct_batch_device(const(short)* coeffs, long coeff_stride, const(ubyte)* max_zag, long zag_stride,
                                                 ubyte* out_, long out_pitch, long out_stride,
                                                 int width, int height, int scan_type, int out_comps, int count, void* stream);
    int  gamut_hip_jpeg_decode_coeffs(const(ubyte)* data, size_t len, gamut_hip_jpeg_frame* out_);
    void gamut_hip_jpeg_frame_free(gamut_hip_jpeg_frame* f);
    int  gamut_hip_jpeg_read_header(const(ubyte)* data, size_t len, gamut_hip_jpeg_frame* out_);
    int  gamut_hip_jpeg_scan_layout(const(ubyte)* data, size_t len, gamut_hip_jpeg_frame* info, int* segments, ulong* entropy_bytes);
    int  gamut_hip_jpeg_entropy_decode_device(const(ubyte*)* data, const(size_t)* len, int count,
                                              const(long)* coeff_offset, const(long)* zag_offset,
                                              short* coeffs, ubyte* max_zag, uint* status_dev,
                                              gamut_hip_jpeg_frame* info, int* status_host, void* stream);
    int  gamut_hip_jpeg_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, int req_comps,
                                            const(long)* out_offset, ubyte* out_, gamut_hip_jpeg_frame* info, int* status_host,
                                            uint* status_dev, void* stream);
    int  gamut_hip_jpeg_decode_coeffs_batch(const(ubyte*)* data, const(size_t)* len, int count,
                                            gamut_hip_jpeg_frame* out_, int* status, int threads);
    ubyte* gamut_hip_decompress_jpeg_image_from_memory(const(ubyte)* data, size_t len, int* width, int* height, int* actual_comps,
                                                       float* pixelAspectRatio, float* dotsPerInchY, int req_comps);
    // C linkage (this alias sits inside extern(C)); D's bool is one byte = the header's unsigned char
    alias gamut_hip_jpeg_stream_read_func = int function(void* pBuf, int max_bytes_to_read, bool* pEOF_flag, void* userData);
    ubyte* gamut_hip_decompress_jpeg_image_from_stream(gamut_hip_jpeg_stream_read_func rfn, void* userData, int* width, int* height,
                                                       int* actual_comps, float* pixelAspectRatio, float* dotsPerInchY, int req_comps);

    // ---- stbdec.d ------------------------------------------------------------------------------------------------
    struct gamut_hip_png_desc { const(ubyte)* raw; ubyte* out_; uint raw_len, x, y; int img_n, out_n, depth, color; }
    int gamut_hip_png_defilter_device(const(gamut_hip_png_desc)* descs, int count, uint* status, void* stream);
    int gamut_hip_png_defilter_batch_device(const(ubyte)* raw, long raw_stride, uint raw_len, ubyte* out_, long out_stride,
                                            uint x, uint y, int img_n, int out_n, int depth, int color, int count, uint* status, void* stream);
    ubyte*  gamut_hip_stbi_load_from_memory(const(ubyte)* data, size_t len, int* x, int* y, int* comp, int req_comp,
                                            float* ppmX, float* ppmY, float* pixelRatio);
    ushort* gamut_hip_stbi_load_16_from_memory(const(ubyte)* data, size_t len, int* x, int* y, int* comp, int req_comp,
                                               float* ppmX, float* ppmY, float* pixelRatio);
    int gamut_hip_png_is16(const(ubyte)* data, size_t len);
    // same layout as stbi_io_callbacks (stbdec.d:408-419) -- three pointers -- but the members are C-linkage function pointers
    struct gamut_hip_stbi_io_callbacks
    {
        int  function(void* user, char* data, int size) read;
        void function(void* user, int n) skip;
        int  function(void* user) eof;
    }
    ubyte*  gamut_hip_stbi_load_from_callbacks(const(gamut_hip_stbi_io_callbacks)* clbk, void* user, int* x, int* y, int* comp, int req_comp,
                                               float* ppmX, float* ppmY, float* pixelRatio);
    ushort* gamut_hip_stbi_load_16_from_callbacks(const(gamut_hip_stbi_io_callbacks)* clbk, void* user, int* x, int* y, int* comp, int req_comp,
                                                  float* ppmX, float* ppmY, float* pixelRatio);
    int gamut_hip_stbi_png_is16_from_callbacks(const(gamut_hip_stbi_io_callbacks)* clbk, void* user);   // header only; rewind afterwards (png.d:50-62)

    struct gamut_hip_inflate_desc { const(ubyte)* src; ubyte* dst; uint src_len, dst_cap; }
    int gamut_hip_inflate_batch_device(const(gamut_hip_inflate_desc)* descs, int count, uint* out_len_dev, uint* status_dev, void* stream);
    int gamut_hip_inflate_batch_device_sliced(const(gamut_hip_inflate_desc)* descs, int count, uint* out_len_dev, uint* status_dev,
                                              uint slice_bytes, void* stream);
    struct gamut_hip_png_info { uint width, height; int channels_in_file, channels, bits;
                                float pixels_per_meter_x, pixels_per_meter_y, pixel_aspect_ratio; }
    int gamut_hip_png_read_header(const(ubyte)* data, size_t len, gamut_hip_png_info* info);
    int gamut_hip_png_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, int req_comp, int bits,
                                          const(long)* out_offset, ubyte* out_, gamut_hip_png_info* info, int* status_host,
                                          int threads, void* stream);

    // ---- qoi.d ---------------------------------------------------------------------------------------------------
    struct gamut_hip_qoi_desc { uint width, height; ubyte channels, colorspace; }
    void* gamut_hip_qoi_decode(const(void)* data, int size, gamut_hip_qoi_desc* desc, int channels);
    int   gamut_hip_qoi_read_header(const(void)* data, int size, gamut_hip_qoi_desc* desc);
    int   gamut_hip_qoi_decode_batch_device(const(ubyte*)* data, const(int)* size, int count, int channels,
                                            const(long)* out_offset, ubyte* out_, gamut_hip_qoi_desc* descs, int* status_host, void* stream);
    int   gamut_hip_qoi_decode_resident_device(const(ubyte)* blob, long blob_len, const(long)* begin, const(int)* size,
                                               const(gamut_hip_qoi_desc)* descs, int count, int channels,
                                               const(long)* out_offset, ubyte* out_, void* stream);
    long  gamut_hip_qoi_encode_bound(const(gamut_hip_qoi_desc)* desc);
    void* gamut_hip_qoi_encode(const(void)* data, const(gamut_hip_qoi_desc)* desc, int pitch_bytes, int* out_len);
    int   gamut_hip_qoi_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(gamut_hip_qoi_desc)* descs,
                                            int count, const(long)* out_offset, ubyte* out_, long* out_len,
                                            int* status_host, void* stream);
    long  gamut_hip_jpeg_encode_bound(int width, int height, int comp, int quality);
    void* gamut_hip_jpeg_encode(const(void)* data, int width, int height, int comp, int pitch, int quality, int* out_len);
    // stbi_write_func (stb_image_write.d) with C linkage
    alias gamut_hip_jpeg_write_func = void function(void* context, const(void)* data, int size);
    int   gamut_hip_jpeg_write_to_func(gamut_hip_jpeg_write_func func, void* context, int x, int y, int comp, const(void)* data,
                                       int pitch, int quality);
    int   gamut_hip_jpeg_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(int)* width, const(int)* height,
                                             const(int)* comp, const(int)* quality, int count, const(long)* out_offset, ubyte* out_,
                                             long* out_len, int* status_host, void* stream);
    // PNG encode: the reference's container and filter stream around a GPU-built zlib stream
    long  gamut_hip_png_encode_bound(int width, int height, int comp, int is16bit);
    void* gamut_hip_png_write_to_mem(const(void)* pixels, int stride_bytes, int x, int y, int n, int* out_len, int is16bit,
                                     int force_filter, int compression_level);
    int   gamut_hip_png_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(int)* width, const(int)* height,
                                            const(int)* comp, const(int)* is16bit, const(int)* force_filter, const(int)* level,
                                            int count, const(long)* out_offset, ubyte* out_, long* out_len, int* status_host,
                                            void* stream);

    // BMP: stbi__bmp_load / write_bmp on the GPU (codecs/stbdec.d:2112-2512, codecs/bmpenc.d, plugins/bmp.d)
    struct gamut_hip_bmp_info { int width, height, bpp, header_size, compression, channels_in_file, top_down, pixel_offset, palette_size;
                                uint mask_r, mask_g, mask_b, mask_a; float pixels_per_meter_x, pixels_per_meter_y, pixel_aspect_ratio; }
    int   gamut_hip_bmp_read_header(const(ubyte)* data, size_t len, gamut_hip_bmp_info* info);
    int   gamut_hip_bmp_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, int req_comp, const(long)* out_offset,
                                            ubyte* out_, gamut_hip_bmp_info* info, int* status_host, void* stream);
    float gamut_hip_bmp_last_decode_kernel_ms();
    long  gamut_hip_bmp_encode_bound(int width, int height, int comp);
    int   gamut_hip_bmp_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(int)* width, const(int)* height,
                                            const(int)* comp, const(int)* ppm_x, const(int)* ppm_y, int count, const(long)* out_offset,
                                            ubyte* out_, long* out_len, int* status_host, void* stream);
    void* gamut_hip_bmp_write_to_mem(const(void)* data, int pitch, int w, int h, int comp, int ppm_x, int ppm_y, int* out_len);

    // GIF: GIFDecoder + loadGIF on the GPU, every frame composited into a layer (codecs/gif.d, plugins/gif.d:57-103)
    struct gamut_hip_gif_info { int width, height, layers, is_gif89; float pixel_aspect_ratio, fps; }
    int   gamut_hip_gif_read_header(const(ubyte)* data, size_t len, gamut_hip_gif_info* info);
    int   gamut_hip_gif_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, const(long)* out_offset,
                                            const(long)* out_capacity, ubyte* out_, gamut_hip_gif_info* info, int* status_host, void* stream);
    float gamut_hip_gif_last_decode_kernel_ms();
    float gamut_hip_gif_last_kernel_ms(int which);
    // GIF encode: saveGIF over msf_gif (plugins/gif.d:105-147, codecs/msf_gif.d), every layer a frame, byte for byte
    long  gamut_hip_gif_encode_bound(int width, int height, int frames);
    int   gamut_hip_gif_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(long)* src_layer_offset,
                                            const(int)* width, const(int)* height, const(int)* frames,
                                            const(int)* centiseconds, const(int)* max_bit_depth, const(int)* alpha_threshold,
                                            int count, const(long)* out_offset, ubyte* out_, long* out_len, int* status_host,
                                            void* stream);
    void* gamut_hip_gif_write_to_mem(const(void)* data, int pitch, long layer_offset, int w, int h, int frames, int centiseconds,
                                     int max_bit_depth, int alpha_threshold, int* out_len);
    float gamut_hip_gif_last_encode_kernel_ms(int which);

    // TGA: TGADecoder.getImageInfo / decodeImage on the GPU (codecs/tga.d:283-647, plugins/tga.d).  read_header gives two
    // verdicts: info.detected is detectTGA's, the return value the load's.  Deviation: width * height * components > int.max is refused.
    struct gamut_hip_tga_info { int width, height, bpp, image_type, rle, indexed, rgb16, channels_in_file, bottom_up, palette_start, palette_len,
                                cmap_size, data_offset, detected; }
    int   gamut_hip_tga_read_header(const(ubyte)* data, size_t len, gamut_hip_tga_info* info);
    int   gamut_hip_tga_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, int req_comp, const(long)* out_offset,
                                            ubyte* out_, gamut_hip_tga_info* info, int* status_host, void* stream);
    int   gamut_hip_tga_rle_window();
    float gamut_hip_tga_last_decode_kernel_ms();
    // SQZ decode (SQZ_decode codecs/sqz.d:2253-2296, loadSQZ plugins/sqz.d:43-133).  decode_coeffs is the bit-serial front end on the host
    // (coefficients as the reference holds them after SQZ_decode_round_coefficients: sign-magnitude, bit 0 the sign), reconstruct_batch_device
    // the back end on the GPU (IDWT and colour; `coeffs` is a working buffer, unspecified after the call), decode_batch_device both from files.
    struct gamut_hip_sqz_info { int width, height, planes, color_mode, levels, scan_order, subsampling, pixel_type, detected; }
    struct gamut_hip_sqz_desc { int width, height, color_mode, levels; long coeff_offset; }
    int   gamut_hip_sqz_read_header(const(ubyte)* data, size_t len, gamut_hip_sqz_info* info);
    int   gamut_hip_sqz_decode_coeffs(const(ubyte)* data, size_t len, short* planes, size_t capacity, gamut_hip_sqz_info* info);
    int   gamut_hip_sqz_reconstruct_batch_device(const(short)* coeffs, const(gamut_hip_sqz_desc)* descs, int count, const(long)* out_offset,
                                                 ubyte* out_, int* status_host, void* stream);
    int   gamut_hip_sqz_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, const(long)* out_offset, ubyte* out_,
                                            gamut_hip_sqz_info* info, int* status_host, void* stream);
    const(ubyte)* gamut_hip_sqz_linear_to_srgb_table();
    float gamut_hip_sqz_last_decode_stage_ms(int stage);
    // SQZ read on the device: the front end as HIP kernels, one workgroup per file; files in host memory -> coefficients in device memory,
    // value for value those of decode_coeffs.  set_reader(0 host / 1 device) chooses what decode_batch_device and the Image layer run; it
    // returns the previous value.
    int   gamut_hip_sqz_read_batch_device(const(ubyte*)* data, const(size_t)* len, int count, short* coeffs, const(long)* coeff_offset,
                                          gamut_hip_sqz_info* info, int* status_host, void* stream);
    int   gamut_hip_sqz_set_reader(int which);
    int   gamut_hip_sqz_read_window();
    long  gamut_hip_sqz_set_read_chunk(long coefficients);
    float gamut_hip_sqz_last_read_stage_ms(int stage);
    // SQZ encode (SQZ_encode codecs/sqz.d:2208-2240, saveSQZ plugins/sqz.d:141-201).  analyze_batch_device is the front half on the GPU (colour
    // transform, DWT, sign-magnitude: the coefficient buffer reconstruct_batch_device consumes), dwt_batch_device the same fed with int16
    // planes, encode_coeffs the bit-plane writer on the host, encode_batch_device both: device pixels -> files in HOST memory.
    struct gamut_hip_sqz_encode_desc { int width, height, color_mode, levels, scan_order, subsampling; long budget; }
    long  gamut_hip_sqz_budget_from_flags(int width, int height, int flags);
    int   gamut_hip_sqz_analyze_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(gamut_hip_sqz_encode_desc)* descs, int count,
                                             short* coeffs, const(long)* coeff_offset, int* status_host, void* stream);
    int   gamut_hip_sqz_dwt_batch_device(const(short)* planes_in, const(gamut_hip_sqz_encode_desc)* descs, int count, short* coeffs,
                                         const(long)* coeff_offset, int* status_host, void* stream);
    int   gamut_hip_sqz_encode_coeffs(const(short)* planes, const(gamut_hip_sqz_encode_desc)* desc, ubyte* dst, long* len);
    int   gamut_hip_sqz_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(gamut_hip_sqz_encode_desc)* descs, int count,
                                            const(long)* out_offset, ubyte* out_, long* out_len, int* status_host, void* stream);
    void* gamut_hip_sqz_write_to_mem(const(void)* data, int pitch, const(gamut_hip_sqz_encode_desc)* desc, int* out_len);
    float gamut_hip_sqz_last_encode_stage_ms(int stage);
    // SQZ write on the device: the bit-plane writer as HIP kernels.  write_batch_device takes coefficient buffers in DEVICE memory (as
    // analyze_batch_device leaves them) and leaves the files in DEVICE memory; encode_batch_to_device is the front half followed by it.
    // set_writer(0 host / 1 device) chooses what encode_batch_device, write_to_mem and the Image layer run; it returns the previous value.
    int   gamut_hip_sqz_write_batch_device(const(short)* coeffs, const(long)* coeff_offset, const(gamut_hip_sqz_encode_desc)* descs, int count,
                                           const(long)* out_offset, ubyte* out_, long* out_len, int* status_host, void* stream);
    int   gamut_hip_sqz_encode_batch_to_device(const(ubyte*)* src, const(long)* src_pitch, const(gamut_hip_sqz_encode_desc)* descs, int count,
                                               const(long)* out_offset, ubyte* out_, long* out_len, int* status_host, void* stream);
    int   gamut_hip_sqz_scan_order(int order, int width, int height, ushort* xy);
    int   gamut_hip_sqz_write_chunk();
    float gamut_hip_sqz_last_write_stage_ms(int stage);
    int   gamut_hip_sqz_set_writer(int which);
    // TGA encode: TGAEncoder as saveTGA drives it (codecs/tga.d:57-281, plugins/tga.d:128-150), byte for byte; comp is the source's
    // channel count (1 l8, 2 la8, 3 rgb8, 4 rgba8).  Deviations: width or height 0 and a bound above int.max are refused.
    long  gamut_hip_tga_encode_bound(int width, int height, int comp);
    int   gamut_hip_tga_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(int)* width, const(int)* height,
                                            const(int)* comp, const(int)* rle, int count, const(long)* out_offset, ubyte* out_,
                                            long* out_len, int* status_host, void* stream);
    void* gamut_hip_tga_write_to_mem(const(void)* data, int pitch, int w, int h, int comp, int rle, int* out_len);
    int   gamut_hip_tga_encode_window();
    float gamut_hip_tga_last_encode_kernel_ms();
    float gamut_hip_tga_last_encode_stage_ms(int stage);
    // DDS / BC7 encode: saveDDS (plugins/dds.d:47-216) with bc7enc16_compress_block on its default parameters, byte for byte; comp
    // is the source's channel count (1 l8, 2 la8, 3 rgb8, 4 rgba8).  Deviation: a file above int.max bytes is refused.
    long  gamut_hip_dds_encode_bound(int width, int height, int comp);
    int   gamut_hip_dds_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(int)* width, const(int)* height,
                                            const(int)* comp, int count, const(long)* out_offset, ubyte* out_, long* out_len,
                                            int* status_host, void* stream);
    int   gamut_hip_bc7_encode_blocks_device(const(ubyte)* rgba_tiles, long n, ubyte* out_, void* stream);
    void* gamut_hip_dds_write_to_mem(const(void)* data, int pitch, int width, int height, int comp, int* out_len);
    float gamut_hip_dds_last_encode_kernel_ms();

    // QOIX, 8-bit rgb / rgba: qoix_lz4_decode (plugins/qoix.d:350-473), LZ4_decompress_fast (codecs/lz4.d:760-978) and qoix_decode
    // (codecs/qoi2avg.d:624-897) on the GPU.  read_header: info.detected is detectQOIX's verdict, the return value the load's
    // (GAMUT_HIP_ERR_UNSUPPORTED for the grey and 10-bit codecs, which are not built yet).  Deviations, each GAMUT_HIP_ERR_DECODE: an LZ4
    // read past the file's end; LZ4 offset 0 or a match from before the first output byte; an executed END opcode; an op byte read at
    // index >= size.
    struct gamut_hip_qoix_info { int width, height, version_, channels, bitdepth, colorspace, compression; float pixel_aspect_ratio, resolution_y;
                                 int orig, pixel_type, detected; }
    int   gamut_hip_qoix_read_header(const(ubyte)* data, size_t len, gamut_hip_qoix_info* info);
    int   gamut_hip_qoix_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, int channels, const(long)* out_offset,
                                             ubyte* out_, gamut_hip_qoix_info* info, int* status_host, void* stream);
    void* gamut_hip_qoix_lz4_decode(const(void)* data, int size, gamut_hip_qoix_info* info, int flags, int* decoded_type);
    int   gamut_hip_qoix_row_capacity();
    float gamut_hip_qoix_last_decode_kernel_ms();
    float gamut_hip_qoix_last_decode_stage_ms(int stage);
    // QOI-Plane (8-bit files with 1 or 2 channels, codecs/qoiplane.d:377-541) behind a process-wide switch: set_plane(0 | 1) returns the
    // previous value (any other argument changes nothing); the initial value is GAMUT_HIP_QOIX_PLANE=0|1, default 0 (such files are
    // GAMUT_HIP_ERR_UNSUPPORTED).  On: l8 / la8 decode, channels 1 / 2 accepted for grey files, and the encode entries take
    // descriptions with 1 / 2 channels (QOI-Plane, qoiplane_encode).
    int   gamut_hip_qoix_set_plane(int on);
    int   gamut_hip_qoix_plane_row_capacity();
    float gamut_hip_qoix_last_plane_kernel_ms();
    // QOIX encode: qoix_lz4_encode as saveQOIX drives it for 8-bit rgb / rgba (plugins/qoix.d:156-339, codecs/qoi2avg.d:376-615,
    // codecs/lz4.d:289-554), byte for byte.  mode 0: LZ4 when lz4Size + 4 < datalen, 1: always stored.  Deviations: width * channels bytes
    // of a row are read whatever the pitch is; a bound above 2^31 - 1 is refused.
    struct gamut_hip_qoix_desc { int width, height, channels, colorspace, mode; float pixel_aspect_ratio, resolution_y; }
    long  gamut_hip_qoix_encode_bound(const(gamut_hip_qoix_desc)* desc);
    int   gamut_hip_qoix_encode_batch_device(const(ubyte*)* src, const(long)* src_pitch, const(gamut_hip_qoix_desc)* descs, int count,
                                             const(long)* out_offset, ubyte* out_, long* out_len, int* status_host, void* stream);
    void* gamut_hip_qoix_write_to_mem(const(void)* data, int pitch, const(gamut_hip_qoix_desc)* desc, int* out_len);
    int   gamut_hip_qoix_encode_window();
    int   gamut_hip_qoix_plane_encode_segment();
    int   gamut_hip_lz4_compress_bound(int n);
    int   gamut_hip_lz4_compress_batch_device(const(ubyte*)* src, const(int)* len, int count, const(long)* out_offset, ubyte* out_,
                                              long* out_len, int* status_host, void* stream);
    float gamut_hip_qoix_last_encode_kernel_ms();
    float gamut_hip_qoix_last_encode_stage_ms(int stage);
    float gamut_hip_qoix_last_plane_encode_stage_ms(int stage);

    // ---- any of the three formats, one call (image.d:1045-1061 identifyFormatFromStream + g_plugins[fif].loadProc, batched) ----
    struct gamut_hip_image_info { int format, width, height, channels_in_file, channels; }
    int gamut_hip_identify_format(const(ubyte)* data, size_t len);
    int gamut_hip_decode_batch_device(const(ubyte*)* data, const(size_t)* len, int count, int req_comps,
                                      const(long)* out_offset, ubyte* out_, gamut_hip_image_info* info, int* status_host, void* stream);

    // ---- multi-GPU: image-index round-robin and the gather of decoded outputs over RCCL ----------------------------
    int  gamut_hip_shard_owner(long image_index, int world);
    long gamut_hip_shard_count(int rank, int world, long total_images);
    long gamut_hip_shard_local_index(long image_index, int world);
    long gamut_hip_shard_global_index(long local_index, int rank, int world);
    int  gamut_hip_host_threads();
    struct gamut_hip_comm;
    int  gamut_hip_comm_get_unique_id(void* id128);
    int  gamut_hip_comm_init(gamut_hip_comm** comm, int world, int rank, const(void)* id128);
    void gamut_hip_comm_destroy(gamut_hip_comm* comm);
    int  gamut_hip_comm_rank(const(gamut_hip_comm)* comm);
    int  gamut_hip_comm_world(const(gamut_hip_comm)* comm);
    int  gamut_hip_gather_outputs_device(gamut_hip_comm* comm, const(void)* local, long local_stride, long bytes_per_image,
                                         long total_images, void* dst, long dst_stride, int root, void* stream);

    // ---- struct layouts: the numbers gcc prints for include/gamut_hip.h (tests/c/abi_layout.c); a D compiler checks them the first time
    //      this file is built, tests/test_capi_cpu.py::test_d_binding_struct_layouts checks them against the C compiler every run -------------
    static assert(gamut_hip_jpeg_desc.sizeof == 48 && gamut_hip_jpeg_desc.coeffs.offsetof == 0 && gamut_hip_jpeg_desc.max_zag.offsetof == 8 && gamut_hip_jpeg_desc.out_.offsetof == 16 && gamut_hip_jpeg_desc.out_pitch.offsetof == 24 && gamut_hip_jpeg_desc.width.offsetof == 32 && gamut_hip_jpeg_desc.height.offsetof == 36 && gamut_hip_jpeg_desc.scan_type.offsetof == 40 && gamut_hip_jpeg_desc.out_comps.offsetof == 44);
    static assert(gamut_hip_jpeg_frame.sizeof == 56 && gamut_hip_jpeg_frame.width.offsetof == 0 && gamut_hip_jpeg_frame.height.offsetof == 4 && gamut_hip_jpeg_frame.comps.offsetof == 8 && gamut_hip_jpeg_frame.scan_type.offsetof == 12 && gamut_hip_jpeg_frame.mcus_per_row.offsetof == 16 && gamut_hip_jpeg_frame.mcus_per_col.offsetof == 20 && gamut_hip_jpeg_frame.blocks_per_mcu.offsetof == 24 && gamut_hip_jpeg_frame.coeffs.offsetof == 32 && gamut_hip_jpeg_frame.max_zag.offsetof == 40 && gamut_hip_jpeg_frame.pixel_aspect_ratio.offsetof == 48 && gamut_hip_jpeg_frame.dpi_y.offsetof == 52);
    static assert(gamut_hip_png_desc.sizeof == 48 && gamut_hip_png_desc.raw.offsetof == 0 && gamut_hip_png_desc.out_.offsetof == 8 && gamut_hip_png_desc.raw_len.offsetof == 16 && gamut_hip_png_desc.x.offsetof == 20 && gamut_hip_png_desc.y.offsetof == 24 && gamut_hip_png_desc.img_n.offsetof == 28 && gamut_hip_png_desc.out_n.offsetof == 32 && gamut_hip_png_desc.depth.offsetof == 36 && gamut_hip_png_desc.color.offsetof == 40);
    static assert(gamut_hip_stbi_io_callbacks.sizeof == 24 && gamut_hip_stbi_io_callbacks.read.offsetof == 0 && gamut_hip_stbi_io_callbacks.skip.offsetof == 8 && gamut_hip_stbi_io_callbacks.eof.offsetof == 16);
    static assert(gamut_hip_inflate_desc.sizeof == 24 && gamut_hip_inflate_desc.src.offsetof == 0 && gamut_hip_inflate_desc.dst.offsetof == 8 && gamut_hip_inflate_desc.src_len.offsetof == 16 && gamut_hip_inflate_desc.dst_cap.offsetof == 20);
    static assert(gamut_hip_png_info.sizeof == 32 && gamut_hip_png_info.width.offsetof == 0 && gamut_hip_png_info.height.offsetof == 4 && gamut_hip_png_info.channels_in_file.offsetof == 8 && gamut_hip_png_info.channels.offsetof == 12 && gamut_hip_png_info.bits.offsetof == 16 && gamut_hip_png_info.pixels_per_meter_x.offsetof == 20 && gamut_hip_png_info.pixels_per_meter_y.offsetof == 24 && gamut_hip_png_info.pixel_aspect_ratio.offsetof == 28);
    static assert(gamut_hip_qoi_desc.sizeof == 12 && gamut_hip_qoi_desc.width.offsetof == 0 && gamut_hip_qoi_desc.height.offsetof == 4 && gamut_hip_qoi_desc.channels.offsetof == 8 && gamut_hip_qoi_desc.colorspace.offsetof == 9);
    static assert(gamut_hip_image_info.sizeof == 20 && gamut_hip_image_info.format.offsetof == 0 && gamut_hip_image_info.width.offsetof == 4 && gamut_hip_image_info.height.offsetof == 8 && gamut_hip_image_info.channels_in_file.offsetof == 12 && gamut_hip_image_info.channels.offsetof == 16);
    // (the TGA struct's numbers are the ones tests/c/tga_abi_layout.c prints; tests/test_tga_cpu.py compares them every run)
    static assert(56 == gamut_hip_tga_info.sizeof && 0 == gamut_hip_tga_info.width.offsetof && 4 == gamut_hip_tga_info.height.offsetof && 8 == gamut_hip_tga_info.bpp.offsetof && 12 == gamut_hip_tga_info.image_type.offsetof && 16 == gamut_hip_tga_info.rle.offsetof && 20 == gamut_hip_tga_info.indexed.offsetof && 24 == gamut_hip_tga_info.rgb16.offsetof && 28 == gamut_hip_tga_info.channels_in_file.offsetof && 32 == gamut_hip_tga_info.bottom_up.offsetof && 36 == gamut_hip_tga_info.palette_start.offsetof && 40 == gamut_hip_tga_info.palette_len.offsetof && 44 == gamut_hip_tga_info.cmap_size.offsetof && 48 == gamut_hip_tga_info.data_offset.offsetof && 52 == gamut_hip_tga_info.detected.offsetof);
    // (the QOIX struct's numbers are the ones tests/c/qoix_abi_layout.c prints; tests/test_qoix_cpu.py compares them every run.  `version` is a
    //  D keyword: the field is version_ here)
    static assert(48 == gamut_hip_qoix_info.sizeof && 0 == gamut_hip_qoix_info.width.offsetof && 4 == gamut_hip_qoix_info.height.offsetof && 8 == gamut_hip_qoix_info.version_.offsetof && 12 == gamut_hip_qoix_info.channels.offsetof && 16 == gamut_hip_qoix_info.bitdepth.offsetof && 20 == gamut_hip_qoix_info.colorspace.offsetof && 24 == gamut_hip_qoix_info.compression.offsetof && 28 == gamut_hip_qoix_info.pixel_aspect_ratio.offsetof && 32 == gamut_hip_qoix_info.resolution_y.offsetof && 36 == gamut_hip_qoix_info.orig.offsetof && 40 == gamut_hip_qoix_info.pixel_type.offsetof && 44 == gamut_hip_qoix_info.detected.offsetof);
    // (the SQZ structs' numbers are the ones tests/c/sqz_abi_layout.c prints; tests/test_sqz_cpu.py compares them every run)
    static assert(36 == gamut_hip_sqz_info.sizeof && 0 == gamut_hip_sqz_info.width.offsetof && 4 == gamut_hip_sqz_info.height.offsetof && 8 == gamut_hip_sqz_info.planes.offsetof && 12 == gamut_hip_sqz_info.color_mode.offsetof && 16 == gamut_hip_sqz_info.levels.offsetof && 20 == gamut_hip_sqz_info.scan_order.offsetof && 24 == gamut_hip_sqz_info.subsampling.offsetof && 28 == gamut_hip_sqz_info.pixel_type.offsetof && 32 == gamut_hip_sqz_info.detected.offsetof);
    static assert(24 == gamut_hip_sqz_desc.sizeof && 0 == gamut_hip_sqz_desc.width.offsetof && 4 == gamut_hip_sqz_desc.height.offsetof && 8 == gamut_hip_sqz_desc.color_mode.offsetof && 12 == gamut_hip_sqz_desc.levels.offsetof && 16 == gamut_hip_sqz_desc.coeff_offset.offsetof);
    // (the SQZ encode struct's numbers are the ones tests/c/sqz_encode_abi_layout.c prints; tests/test_sqz_encode_cpu.py compares them every run)
    static assert(32 == gamut_hip_sqz_encode_desc.sizeof && 0 == gamut_hip_sqz_encode_desc.width.offsetof && 4 == gamut_hip_sqz_encode_desc.height.offsetof && 8 == gamut_hip_sqz_encode_desc.color_mode.offsetof && 12 == gamut_hip_sqz_encode_desc.levels.offsetof && 16 == gamut_hip_sqz_encode_desc.scan_order.offsetof && 20 == gamut_hip_sqz_encode_desc.subsampling.offsetof && 24 == gamut_hip_sqz_encode_desc.budget.offsetof);
    // (the QOIX encode struct's numbers are the ones tests/c/qoix_encode_abi_layout.c prints; tests/test_qoix_encode_cpu.py compares them every run)
    static assert(28 == gamut_hip_qoix_desc.sizeof && 0 == gamut_hip_qoix_desc.width.offsetof && 4 == gamut_hip_qoix_desc.height.offsetof && 8 == gamut_hip_qoix_desc.channels.offsetof && 12 == gamut_hip_qoix_desc.colorspace.offsetof && 16 == gamut_hip_qoix_desc.mode.offsetof && 20 == gamut_hip_qoix_desc.pixel_aspect_ratio.offsetof && 24 == gamut_hip_qoix_desc.resolution_y.offsetof);
    // (the BMP struct's numbers are the ones tests/c/bmp_abi_layout.c prints; tests/test_bmp_cpu.py compares them every run)
    static assert(64 == gamut_hip_bmp_info.sizeof && 0 == gamut_hip_bmp_info.width.offsetof && 4 == gamut_hip_bmp_info.height.offsetof && 8 == gamut_hip_bmp_info.bpp.offsetof && 12 == gamut_hip_bmp_info.header_size.offsetof && 16 == gamut_hip_bmp_info.compression.offsetof && 20 == gamut_hip_bmp_info.channels_in_file.offsetof && 24 == gamut_hip_bmp_info.top_down.offsetof && 28 == gamut_hip_bmp_info.pixel_offset.offsetof && 32 == gamut_hip_bmp_info.palette_size.offsetof && 36 == gamut_hip_bmp_info.mask_r.offsetof && 40 == gamut_hip_bmp_info.mask_g.offsetof && 44 == gamut_hip_bmp_info.mask_b.offsetof && 48 == gamut_hip_bmp_info.mask_a.offsetof && 52 == gamut_hip_bmp_info.pixels_per_meter_x.offsetof && 56 == gamut_hip_bmp_info.pixels_per_meter_y.offsetof && 60 == gamut_hip_bmp_info.pixel_aspect_ratio.offsetof);
    // (the GIF struct's numbers are the ones tests/c/gif_abi_layout.c prints; tests/test_gif_cpu.py compares them every run)
    static assert(24 == gamut_hip_gif_info.sizeof && 0 == gamut_hip_gif_info.width.offsetof && 4 == gamut_hip_gif_info.height.offsetof && 8 == gamut_hip_gif_info.layers.offsetof && 12 == gamut_hip_gif_info.is_gif89.offsetof && 16 == gamut_hip_gif_info.pixel_aspect_ratio.offsetof && 20 == gamut_hip_gif_info.fps.offsetof);
}

// ================================================================================================================
// The callbacks.  Way (2): five trampolines with C linkage that forward to the reference's extern(D) functions.
// They live next to their targets: the two JPEG ones in plugins/jpeg.d, the three stb ones in codecs/stbdec.d.
// ================================================================================================================

version (GamutHipTrampolines)
{
    import gamut.plugins.jpeg : stream_read_jpeg, stb_stream_write;   // plugins/jpeg.d:167, :180, extern(D)
    import gamut.codecs.stbdec : stb_read, stb_skip, stb_eof, IOAndHandle;   // codecs/stbdec.d:143-165, extern(D)

    extern(C) int gamut_hip_tramp_read_jpeg(void* pBuf, int max_bytes_to_read, bool* pEOF_flag, void* userData) @system
    {
        return stream_read_jpeg(pBuf, max_bytes_to_read, pEOF_flag, userData);
    }
    extern(C) int  gamut_hip_tramp_stb_read(void* user, char* data, int size) @system { return stb_read(user, data, size); }
    extern(C) void gamut_hip_tramp_stb_skip(void* user, int n) @system               { stb_skip(user, n); }
    extern(C) int  gamut_hip_tramp_stb_eof(void* user) @system                        { return stb_eof(user); }
    extern(C) void gamut_hip_tramp_stb_write(void* context, const(void)* data, int size) @system { stb_stream_write(context, data, size); }

    /// what `initSTBCallbacks` (stbdec.d:126-133) becomes for the HIP path
    void initHipSTBCallbacks(IOStream* io, IOHandle handle, IOAndHandle* ioh, gamut_hip_stbi_io_callbacks* cb) @system
    {
        ioh.io = io;
        ioh.handle = handle;
        cb.read = &gamut_hip_tramp_stb_read;
        cb.skip = &gamut_hip_tramp_stb_skip;
        cb.eof  = &gamut_hip_tramp_stb_eof;
    }

    // loadJPEG, plugins/jpeg.d:61 -- the call becomes
    //     ubyte* p = gamut_hip_decompress_jpeg_image_from_stream(&gamut_hip_tramp_read_jpeg, &jio, &width, &height, &actualComp,
    //                                                            &pixelAspectRatio, &dotsPerInchY, requestedComp);
    //     ubyte[] decoded = p is null ? null : p[0 .. cast(size_t) width * height * (requestedComp == -1 ? actualComp : requestedComp)];
    // loadPNG, plugins/png.d:45-89 -- `initSTBCallbacks(io, handle, &ioh, &stb_callback)` becomes
    //     gamut_hip_stbi_io_callbacks cb;  initHipSTBCallbacks(io, handle, &ioh, &cb);
    //     bool is16bit = gamut_hip_stbi_png_is16_from_callbacks(&cb, &ioh) != 0;
    //     ... decoded = gamut_hip_stbi_load_from_callbacks(&cb, &ioh, &width, &height, &components, requestedComp, &ppmX, &ppmY, &pixelRatio);
    // saveJPEG, plugins/jpeg.d:141 -- `stbi_write_jpg_to_func(&stb_stream_write, userPointer, ...)` becomes
    //     int res = gamut_hip_jpeg_write_to_func(&gamut_hip_tramp_stb_write, userPointer, image._width, image._height, components,
    //                                            image._data, image._pitch, quality);
    // savePNG, plugins/png.d:208 -- `stbi_write_png_to_mem(pixels, pitch, width, height, channels, &len, is16Bit, ...)` becomes
    //     ubyte* encoded = cast(ubyte*) gamut_hip_png_write_to_mem(pixels, pitch, width, height, channels, &len, is16Bit,
    //                                                              force_filter, compression_level);
}
