/* sampling_fixture_helper.c -- the C side of scripts/make_sampling_fixtures.py: writes one YCbCr JPEG at a chosen luma sampling with
 * IJG libjpeg and reads its planes back with raw_data_out, the bytes tests/golden/sampling/ pins the device decoder to.
 *
 *   sampling_fixture_helper <in.rgb> <w> <h> <hs> <vs> <quality> <variant> <out.jpg> <out.ycc>
 *
 * in.rgb: w * h * 3 bytes; hs, vs: the luma sampling factors (chroma 1x1); variant: 0 baseline, 1 restart interval of 2 MCUs,
 * 2 progressive; out.ycc: Y (w x h), then Cb and Cr (ceil(w / hs) x ceil(h / vs): libjpeg's downsampled size), packed.
 * Build: gcc -O2 -I<prefix>/include sampling_fixture_helper.c -L<prefix>/lib -ljpeg -Wl,-rpath,<prefix>/lib */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <jpeglib.h>

static void die(const char* what) { fprintf(stderr, "sampling_fixture_helper: %s\n", what); exit(1); }

static unsigned char* read_file(const char* path, size_t n) {
  FILE* f = fopen(path, "rb");
  unsigned char* p = (unsigned char*)malloc(n);
  if (!f || !p || fread(p, 1, n, f) != n) die("cannot read the input");
  fclose(f);
  return p;
}

static void write_jpeg(const unsigned char* rgb, int w, int h, int hs, int vs, int quality, int variant, const char* path) {
  struct jpeg_compress_struct c;
  struct jpeg_error_mgr err;
  FILE* f = fopen(path, "wb");
  if (!f) die("cannot open the JPEG for writing");
  c.err = jpeg_std_error(&err);
  jpeg_create_compress(&c);
  jpeg_stdio_dest(&c, f);
  c.image_width = (JDIMENSION)w; c.image_height = (JDIMENSION)h; c.input_components = 3; c.in_color_space = JCS_RGB;
  jpeg_set_defaults(&c);
  jpeg_set_quality(&c, quality, TRUE);
  c.dct_method = JDCT_ISLOW;
  c.comp_info[0].h_samp_factor = hs; c.comp_info[0].v_samp_factor = vs;
  c.comp_info[1].h_samp_factor = c.comp_info[1].v_samp_factor = 1;
  c.comp_info[2].h_samp_factor = c.comp_info[2].v_samp_factor = 1;
  if (variant == 1) c.restart_interval = 2;
  if (variant == 2) jpeg_simple_progression(&c);
  jpeg_start_compress(&c, TRUE);
  while (c.next_scanline < c.image_height) {
    JSAMPROW row = (JSAMPROW)(rgb + (size_t)c.next_scanline * (size_t)w * 3);
    jpeg_write_scanlines(&c, &row, 1);
  }
  jpeg_finish_compress(&c);
  jpeg_destroy_compress(&c);
  fclose(f);
}

/* the planes as jpeg_read_raw_data returns them, cropped to each component's downsampled size */
static void read_planes(const char* jpg, const char* out, int hs, int vs) {
  struct jpeg_decompress_struct d;
  struct jpeg_error_mgr err;
  FILE* f = fopen(jpg, "rb");
  FILE* o = fopen(out, "wb");
  if (!f || !o) die("cannot open the files of the decode");
  d.err = jpeg_std_error(&err);
  jpeg_create_decompress(&d);
  jpeg_stdio_src(&d, f);
  jpeg_read_header(&d, TRUE);
  d.raw_data_out = TRUE;
  d.out_color_space = JCS_YCbCr;
  d.dct_method = JDCT_ISLOW;
  d.do_fancy_upsampling = FALSE;
  jpeg_start_decompress(&d);
  if (d.num_components != 3 || d.comp_info[0].h_samp_factor != hs || d.comp_info[0].v_samp_factor != vs) die("unexpected sampling");
  {
    const int w = (int)d.output_width, h = (int)d.output_height;
    const int pw[3] = {w, (w + hs - 1) / hs, (w + hs - 1) / hs}, ph[3] = {h, (h + vs - 1) / vs, (h + vs - 1) / vs};
    const int lines = 8 * vs;                   /* luma rows per jpeg_read_raw_data call (one row of MCUs) */
    const int mcus_x = (w + 8 * hs - 1) / (8 * hs), mcus_y = (h + 8 * vs - 1) / (8 * vs);
    const int bufw[3] = {mcus_x * 8 * hs, mcus_x * 8, mcus_x * 8}, bufh[3] = {mcus_y * 8 * vs, mcus_y * 8, mcus_y * 8};
    unsigned char* buf[3];
    JSAMPROW rows[3][16];
    JSAMPARRAY planes[3] = {rows[0], rows[1], rows[2]};
    int c, r, done = 0;
    for (c = 0; c < 3; ++c) {
      buf[c] = (unsigned char*)calloc((size_t)bufw[c] * (size_t)bufh[c], 1);
      if (!buf[c]) die("out of memory");
    }
    while (d.output_scanline < d.output_height) {
      for (r = 0; r < lines; ++r) rows[0][r] = buf[0] + (size_t)(done * lines + r) * (size_t)bufw[0];
      for (c = 1; c < 3; ++c)
        for (r = 0; r < 8; ++r) rows[c][r] = buf[c] + (size_t)(done * 8 + r) * (size_t)bufw[c];
      if (jpeg_read_raw_data(&d, planes, (JDIMENSION)lines) == 0) die("jpeg_read_raw_data returned nothing");
      ++done;
    }
    for (c = 0; c < 3; ++c)
      for (r = 0; r < ph[c]; ++r)
        if (fwrite(buf[c] + (size_t)r * (size_t)bufw[c], 1, (size_t)pw[c], o) != (size_t)pw[c]) die("short write");
    for (c = 0; c < 3; ++c) free(buf[c]);
  }
  jpeg_finish_decompress(&d);
  jpeg_destroy_decompress(&d);
  fclose(f);
  fclose(o);
}

int main(int argc, char** argv) {
  if (argc != 10) die("usage: <in.rgb> <w> <h> <hs> <vs> <quality> <variant> <out.jpg> <out.ycc>");
  {
    const int w = atoi(argv[2]), h = atoi(argv[3]), hs = atoi(argv[4]), vs = atoi(argv[5]), q = atoi(argv[6]), variant = atoi(argv[7]);
    unsigned char* rgb;
    if (w < 1 || h < 1 || w > 8192 || h > 8192 || hs < 1 || hs > 2 || vs < 1 || vs > 2 || variant < 0 || variant > 2) die("bad arguments");
    rgb = read_file(argv[1], (size_t)w * (size_t)h * 3);
    write_jpeg(rgb, w, h, hs, vs, q, variant, argv[8]);
    read_planes(argv[8], argv[9], hs, vs);
    free(rgb);
  }
  return 0;
}
