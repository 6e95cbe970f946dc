/* encode_sampling_fixture_helper -- IJG libjpeg in raw-data mode on three planes (scripts/make_encode_sampling_fixtures.py).
 *
 *   encode_sampling_fixture_helper in.ycc w h hs vs quality out.jpg
 *
 * in.ycc: Y (w x h), Cb, Cr (ceil(w / hs) x ceil(h / vs) each), packed.  The file: jpeg_set_defaults, jpeg_set_quality(q, TRUE), ISLOW,
 * luma sampling hs x vs over 1x1 chroma, raw_data_in.  jpeg_write_raw_data wants whole iMCU rows of whole blocks: the buffers handed to
 * it repeat each plane's last column out to the block grid and its last row below, as libjpeg's own edge expansion does. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <jpeglib.h>

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: %s in.ycc w h hs vs quality out.jpg\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), hs = atoi(argv[4]), vs = atoi(argv[5]), quality = atoi(argv[6]);
  const int cw = (w + hs - 1) / hs, ch = (h + vs - 1) / vs;
  const size_t n = (size_t)w * h + 2 * (size_t)cw * ch;
  unsigned char* in = malloc(n);
  FILE* f = fopen(argv[1], "rb");
  if (!in || !f || fread(in, 1, n, f) != n) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  FILE* out = fopen(argv[7], "wb");
  if (!out) { fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }

  struct jpeg_compress_struct c;
  struct jpeg_error_mgr err;
  c.err = jpeg_std_error(&err);
  jpeg_create_compress(&c);
  jpeg_stdio_dest(&c, out);
  c.image_width = w; c.image_height = h; c.input_components = 3; c.in_color_space = JCS_YCbCr;
  jpeg_set_defaults(&c);
  jpeg_set_quality(&c, quality, TRUE);
  c.dct_method = JDCT_ISLOW;
  c.raw_data_in = TRUE;
#if JPEG_LIB_VERSION >= 70
  c.do_fancy_downsampling = FALSE;
#endif
  c.comp_info[0].h_samp_factor = hs; c.comp_info[0].v_samp_factor = vs;
  c.comp_info[1].h_samp_factor = c.comp_info[1].v_samp_factor = 1;
  c.comp_info[2].h_samp_factor = c.comp_info[2].v_samp_factor = 1;
  jpeg_start_compress(&c, TRUE);

  /* the planes padded to whole iMCUs by replication */
  const int mcus_x = (w + 8 * hs - 1) / (8 * hs), mcus_y = (h + 8 * vs - 1) / (8 * vs);
  const int pw[3] = {mcus_x * 8 * hs, mcus_x * 8, mcus_x * 8}, ph[3] = {mcus_y * 8 * vs, mcus_y * 8, mcus_y * 8};
  const int sw[3] = {w, cw, cw}, sh[3] = {h, ch, ch};
  const unsigned char* src[3] = {in, in + (size_t)w * h, in + (size_t)w * h + (size_t)cw * ch};
  unsigned char* pad[3];
  for (int k = 0; k < 3; ++k) {
    pad[k] = malloc((size_t)pw[k] * ph[k]);
    for (int r = 0; r < ph[k]; ++r)
      for (int x = 0; x < pw[k]; ++x)
        pad[k][(size_t)r * pw[k] + x] = src[k][(size_t)(r < sh[k] ? r : sh[k] - 1) * sw[k] + (x < sw[k] ? x : sw[k] - 1)];
  }
  JSAMPROW rows[3][16];
  JSAMPARRAY planes[3] = {rows[0], rows[1], rows[2]};
  for (int m = 0; m < mcus_y; ++m) {
    for (int k = 0; k < 3; ++k) {
      const int nr = k == 0 ? 8 * vs : 8;
      for (int r = 0; r < nr; ++r) rows[k][r] = pad[k] + (size_t)(m * nr + r) * pw[k];
    }
    if (jpeg_write_raw_data(&c, planes, 8 * vs) != (JDIMENSION)(8 * vs)) { fprintf(stderr, "short write\n"); return 1; }
  }
  jpeg_finish_compress(&c);
  jpeg_destroy_compress(&c);
  fclose(out);
  return 0;
}
