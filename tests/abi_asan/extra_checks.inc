// Hand-written checks appended to the generated driver (tests/test_abi_asan_cpu.py): the validation layer must refuse bad
// arguments with a negative status and a message -- before any HIP call, so this runs on a host without a GPU -- and the
// host-only helpers must give their documented answers.  Built with -fsanitize=address,undefined.
static int extra_checks() {
  int bad = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "extra check failed: %s (line %d)\n", #cond, __LINE__); ++bad; } } while (0)
  char buf[64];
  long long st[5] = {1, 1, 1, 1, 1};
  // dtype / shape / pointer validation of the forward entry points
  EXPECT(iunet_pack_conv3(7, buf, nullptr, buf, 32, 32, 9, 0, nullptr) < 0 && std::strstr(iunet_last_error(), "dtype"));
  EXPECT(iunet_pack_conv3(0, buf, nullptr, buf, 32, 32, 10, 0, nullptr) < 0 && std::strstr(iunet_last_error(), "taps"));
  EXPECT(iunet_conv3_fwd(0, 3, buf, 0, buf, 0, buf, nullptr, nullptr, 1, 0, 4, 4, 32, 32, 2, 0, nullptr) < 0);
  EXPECT(iunet_conv3_fwd(0, 3, buf, 0, buf, 0, buf, nullptr, nullptr, 1, 4, 4, 4, 32, 32, 5, 0, nullptr) < 0 && std::strstr(iunet_last_error(), "epilogue"));
  EXPECT(iunet_conv3_fwd(0, 3, buf, 0, buf, 0, buf, nullptr, nullptr, 1, 4, 4, 4, 32, 32, 2, 9, nullptr) < 0 && std::strstr(iunet_last_error(), "layout"));
  // the retired kernel structures: layouts 0 / 1 and the pack modes without the K16 bit are refused with otherwise valid arguments
  EXPECT(iunet_conv3_fwd(0, 3, buf, 0, buf, 0, buf, nullptr, nullptr, 1, 4, 4, 4, 32, 32, 0, 0, nullptr) < 0 && std::strstr(iunet_last_error(), "layout"));
  EXPECT(iunet_conv3_fwd(0, 3, buf, 0, buf, 0, buf, nullptr, nullptr, 1, 4, 4, 4, 32, 32, 0, 1, nullptr) < 0 && std::strstr(iunet_last_error(), "layout"));
  EXPECT(iunet_pack_conv3(0, buf, nullptr, buf, 32, 32, 9, 0, nullptr) < 0 && std::strstr(iunet_last_error(), "mode"));
  EXPECT(iunet_pack_conv3_elems(32, 32, 9, 1) < 0 && std::strstr(iunet_last_error(), "mode") && iunet_pack_conv3_elems(32, 32, 9, 6) == 32 * 32 * 9);
  // the launch policy (host arithmetic): a fusion exists iff nd == 3 or Cin <= 64; the compact operator where it was packed and qualifies
  { int f = -1;
    EXPECT(iunet_conv3_pick_layout(2, 1, 1, 64, 64, 128, 128) == 2 && iunet_conv3_packs_compact(9, 256) == 1 && iunet_conv3_packs_compact(27, 32) == 0);
    EXPECT(iunet_conv3_plan(2, 1, 1, 64, 64, 128, 64, 0, 1, 1, &f) == 3 && f == 0);     // 2-D, more than 64 input channels: plain on layout 3
    EXPECT(iunet_conv3_plan(2, 1, 1, 64, 64, 64, 64, 0, 1, 1, &f) == 3 && f == 1);
    EXPECT(iunet_conv3_plan(3, 1, 8, 8, 16, 64, 64, 0, 1, 1, &f) == 2 && f == 1);       // 3-D: the fused sums on the padded operator
    EXPECT(iunet_conv3_plan(3, 1, 8, 8, 16, 64, 64, 1, 0, 1, &f) == 3 && f == 1 && iunet_conv3_plan(3, 1, 8, 8, 16, 64, 64, 0, 0, 0, nullptr) == 2); }
  EXPECT(iunet_first_conv_fwd(0, 2, buf, 9, st, buf, 0, buf, nullptr, nullptr, 1, 1, 8, 8, 1, 32, 1, nullptr) < 0);
  EXPECT(iunet_first_conv_fwd(0, 2, buf, 0, st, buf, 0, buf, nullptr, nullptr, 1, 3, 8, 8, 1, 32, 1, nullptr) < 0);       // 2-D needs D == 1
  EXPECT(iunet_maxpool_fwd(0, 2, buf, 0, buf, 0, 12, 1, 1, 4, 4, nullptr) < 0);                                        // C % 8
  EXPECT(iunet_head_fwd(0, buf, 0, 32, buf, buf, 1, nullptr, nullptr, nullptr, st, 1.f, 0, 1, 1, 4, 4, nullptr) < 0);  // ncls 2..10
  EXPECT(iunet_head_fwd(0, buf, 0, 32, buf, buf, 11, nullptr, nullptr, nullptr, st, 1.f, 0, 1, 1, 4, 4, nullptr) < 0);
  // fp32 parity mode
  EXPECT(iunet_f32_pack_conv(buf, buf, nullptr, nullptr, nullptr, nullptr, nullptr, 1e-5f, 48, 8, 27, 0, nullptr) < 0);   // Cout % 32
  EXPECT(iunet_f32_pack_conv(buf, buf, nullptr, nullptr, nullptr, nullptr, nullptr, 1e-5f, 32, 8, 8, 0, nullptr) < 0);    // taps of a conv
  EXPECT(iunet_f32_pack_conv(buf, buf, nullptr, buf, nullptr, nullptr, nullptr, 1e-5f, 32, 8, 27, 0, nullptr) < 0);      // fold needs all four
  EXPECT(iunet_f32_pack_conv_elems(32, 3, 27) == 1LL * 27 * 256 && iunet_f32_pack_conv_elems(33, 3, 27) == 0);
  EXPECT(iunet_f32_conv_fwd(4, buf, 0, st, buf, 0, buf, nullptr, 1, 1, 4, 4, 8, 32, 1, 0, nullptr) < 0);
  EXPECT(iunet_f32_conv_fwd(2, buf, 0, st, buf, 0, buf, nullptr, 1, 2, 4, 4, 8, 32, 1, 0, nullptr) < 0);
  EXPECT(iunet_f32_head_fwd(buf, 0, 32, buf, buf, 12, nullptr, nullptr, nullptr, st, 1.f, 0, 1, 1, 4, 4, nullptr) < 0);
  // volume prediction
  int blk[6] = {0, 0, 0, 4, 4, 9}, loc[6] = {0, 0, 0, 4, 4, 4};
  EXPECT(iunet_blend_accumulate(buf, buf, buf, buf, 8, 8, 8, 2, 4, blk, loc, nullptr) < 0 && std::strstr(iunet_last_error(), "outside"));
  int blk2[6] = {0, 0, 0, 4, 4, 4}, loc2[6] = {2, 0, 0, 6, 4, 4};
  EXPECT(iunet_blend_accumulate(buf, buf, buf, buf, 8, 8, 8, 2, 4, blk2, loc2, nullptr) < 0);
  EXPECT(iunet_gather_block(buf, 8, 8, 8, 9, 0, 0, 4, buf, nullptr) < 0);                                              // block beside the volume
  EXPECT(iunet_colorize(nullptr, 4, buf, 2, buf, nullptr) < 0);
  // host-only arithmetic: scipy's zoom table (see include/iunet.h)
  int tab[4];
  EXPECT(iunet_zoom_nearest_len(8, 0.5) == 4 && iunet_zoom_nearest_len(0, 0.5) == 0);
  EXPECT(iunet_zoom_nearest_table(8, 0.5, tab, 4) == 0 && tab[0] == 0 && tab[3] == 7);
  EXPECT(iunet_zoom_nearest_table(8, 0.5, tab, 3) < 0 && std::strstr(iunet_last_error(), "n_out"));
  EXPECT(iunet_abi_version() >= 1 && iunet_pack_desc_bytes() > 0 && iunet_augment_desc_bytes() > 0);
  EXPECT(iunet_pack_first_conv_elems(32, 1, 27) == 32 * 32);
  return bad;
}

// the error string is thread local: two threads failing differently must each read their own message
static int thread_checks() {
  int bad = 0;
  std::thread a([&] { for (int i = 0; i < 2000; ++i) { iunet_pack_conv3(7, nullptr, nullptr, nullptr, 32, 32, 9, 0, nullptr);
                                                       if (!std::strstr(iunet_last_error(), "dtype")) ++bad; } });
  std::thread b([&] { char buf[8]; for (int i = 0; i < 2000; ++i) { iunet_pack_conv3(0, buf, nullptr, buf, 32, 32, 10, 0, nullptr);
                                                       if (!std::strstr(iunet_last_error(), "taps")) ++bad; } });
  a.join(); b.join();
  return bad;
}
