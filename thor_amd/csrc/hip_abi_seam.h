// hip_abi_seam.h - C ABI, drop-in seam of include/thor_abi.h: encode_frame_lbd / _hbd (enc/encode_frame.h:32-33; part of the translation unit thor_hip.cpp).
#pragma once

static void seam_fatal(const char* msg) {  // fatalerror() convention, common/global.h:38-44
  fprintf(stderr, "Run-time error...\n%s\n...now exiting to system...\n", msg);
  abort();
}

// putbits(n, val) of enc/putbits.c:109-128 for 1 <= n <= 16 (same lazy flush: a full accumulator is only written out
// by the next put, so the caller's (bitbuf, bitrest, bytepos) end up exactly as if the reference had written the bits)
static void stream_put(thor_stream* s, unsigned n, unsigned val) {
  val &= (1u << n) - 1u;
  if (n <= s->bitrest) {
    s->bitbuf |= val << (s->bitrest - n);
    s->bitrest -= n;
  } else {
    const unsigned rest = n - s->bitrest;
    s->bitbuf |= val >> rest;
    if (s->bytepos + 4 > s->bytesize) seam_fatal("Run out of bits in stream buffer.");
    for (int i = 3; i >= 0; --i) s->bitstream[s->bytepos++] = (uint8_t)((s->bitbuf >> (8 * i)) & 0xff);
    s->bitbuf = (val & ((1u << rest) - 1u)) << (32 - rest);
    s->bitrest = 32 - rest;
  }
}

// the sequence parameters of a caller's encoder_info: the shared fields as they are (hip_abi_seq.h: TK_PARAMS_SEAM), the rest by the seam's own rules
static SeqParams seam_params(const thor_encoder_info& ei) {
  const thor_enc_params& src = *ei.params;
  SeqParams dst;
  TK_PARAMS_SEAM(TK_PARAM_COPY)
  dst.width = ei.width; dst.height = ei.height; dst.qp = (int)src.qp;
  dst.HQperiod = THOR_MAX_REF_FRAMES - 1;  // window large enough for any ref_array the caller builds
  dst.dyadic_coding = 1;  // the caller owns the GOP structure; only the window size matters here
  return dst;
}

template <typename PIX> struct SeamState {
  Engine<PIX> eng;
};
template <typename PIX> static std::map<const void*, SeamState<PIX>*>& seams() {
  static std::map<const void*, SeamState<PIX>*> m;
  return m;
}

template <typename PIX> static void encode_frame_impl(struct thor_encoder_info* ei) {
  if (!ei || !ei->params || !ei->orig || !ei->rec || !ei->stream) seam_fatal("encode_frame: null encoder_info member");
  if ((ei->params->bitdepth > 8) != (sizeof(PIX) == 2)) seam_fatal("thor_hip: frame sample size does not match params->bitdepth");
  const thor_enc_params& ep = *ei->params;
  thor_frame_info& fi = ei->frame_info;
  SeamState<PIX>*& st = seams<PIX>()[ei];
  if (!st) {
    SeqParams s = seam_params(*ei);
    if (ep.subsample != 420 || (ep.log2_sb_size != 6 && ep.log2_sb_size != 7) || ep.qmtx || ep.max_delta_qp || ep.bitrate || ep.sync)
      seam_fatal("thor_hip: unsupported encoder parameters (need 4:2:0, 64x64 or 128x128 SB, no qmtx / delta-QP / rate control / sync)");
    if (unsupported(s)) seam_fatal("thor_hip: unsupported encoder parameters");
    s.input_bitdepth = s.bitdepth;  // the caller's front end has widened `orig` and keeps `rec` at the internal depth: frames cross the seam as they are
    if (!ensure_init(getenv("THOR_HIP_DEVICE") ? atoi(getenv("THOR_HIP_DEVICE")) : 0)) seam_fatal("thor_hip: HIP device not usable");
    st = new SeamState<PIX>;
    st->eng.raw_frames = true;
    st->eng.external_interp = true;  // the caller interpolates (enc/mainenc.c:353) and hands the frame over
    st->eng.open(s, 1);
  }
  Engine<PIX>& eng = st->eng;
  if (fi.interp_ref > 1) seam_fatal("thor_hip: interp_ref > 1 is not implemented");
  if (fi.num_ref > kMaxRefs) seam_fatal("thor_hip: more than 4 references");
  FrameParams f;
  f.frame_type = fi.frame_type; f.qp = fi.qp; f.num_ref = fi.num_ref; f.frame_num = fi.frame_num; f.interp_ref = fi.interp_ref;
  f.num_intra_modes = fi.num_intra_modes; f.b_level = fi.b_level;
  for (int r = 0; r < fi.num_ref; r++) {
    if (fi.ref_array[r] < -1 || fi.ref_array[r] >= eng.ring_size) seam_fatal("thor_hip: reference index outside the device window");
    f.ref_array[r] = fi.ref_array[r];
    if (fi.ref_array[r] == -1) {  // interpolated frame built by the caller
      if (!ei->interp_frames[0] || !ep.interp_ref) seam_fatal("thor_hip: ref_array -1 without an interpolated frame");
      const thor_yuv_frame& q = *ei->interp_frames[0];
      DevFrame<PIX>& g = eng.st[0].interp;
      auto push = [&](const PIX* hp, int hs, PIX* dp, int ds, int w, int h, int padw, int padh) {
        std::vector<PIX> buf((size_t)(h + 2 * padh) * ds);
        for (int i = -padh; i < h + padh; i++) memcpy(&buf[(size_t)(i + padh) * ds], hp + (ptrdiff_t)i * hs - padw, (w + 2 * padw) * sizeof(PIX));
        backend::h2d(dp - (size_t)padh * ds - padw, buf.data(), (buf.size() - (size_t)(ds - (w + 2 * padw))) * sizeof(PIX));
      };
      if (q.pad_hor_y < kPadY || q.pad_ver_y < kPadY) seam_fatal("thor_hip: interpolated frame padding too small");
      push((const PIX*)q.y, q.stride_y, g.p.y, g.p.sy, ei->width, ei->height, kPadY, kPadY);
      push((const PIX*)q.u, q.stride_c, g.p.u, g.p.sc, ei->width / 2, ei->height / 2, kPadY / 2, kPadY / 2);
      push((const PIX*)q.v, q.stride_c, g.p.v, g.p.sc, ei->width / 2, ei->height / 2, kPadY / 2, kPadY / 2);
      g.frame_num = q.frame_num;
    }
  }
  // lambda_coeff by frame type / B level (enc/encode_frame.c:655-672)
  if (fi.frame_type == F_I) f.lambda_coeff = ep.lambda_coeffI;
  else if (fi.frame_type == F_P) f.lambda_coeff = ep.lambda_coeffP;
  else f.lambda_coeff = fi.b_level == 0 ? ep.lambda_coeffB0 : fi.b_level == 1 ? ep.lambda_coeffB1 : fi.b_level == 2 ? ep.lambda_coeffB2
                                          : fi.b_level == 3 ? ep.lambda_coeffB3 : ep.lambda_coeffB;
  fi.lambda_coeff = f.lambda_coeff;
  fi.lambda = f.lambda_coeff * kSquaredLambdaQP[f.qp];
  fi.prev_qp = fi.qp;
  const thor_yuv_frame& o = *ei->orig;
  eng.upload_planes(0, (const PIX*)o.y, o.stride_y, (const PIX*)o.u, (const PIX*)o.v, o.stride_c);
  eng.st[0].num_encoded = fi.frame_num;  // only used for bookkeeping
  eng.st[0].bit_phase = (8 * (int)ei->stream->bytepos + (32 - (int)ei->stream->bitrest)) & 31;  // get_bit_pos() of the caller's stream
  std::vector<FrameParams> fp(1, f);
  eng.encode_frames(fp);
  // bits -> caller's stream (the caller flushes: enc/mainenc.c:595)
  HostBits& b = eng.st[0].bits;
  {
    int i = 0;
    for (; i + 16 <= b.nbits; i += 16) stream_put(ei->stream, 16, (b.w[i >> 5] >> (16 - (i & 16))) & 0xffffu);
    for (; i < b.nbits; i++) stream_put(ei->stream, 1, (unsigned)b.get(i));
  }
  b.clear();
  // reconstruction -> caller's rec frame
  {
    thor_yuv_frame& r = *ei->rec;
    std::vector<PIX> tmp((size_t)ei->width * ei->height * 3 / 2);
    eng.download_rec(0, tmp.data());
    const int w = ei->width, h = ei->height;
    for (int i = 0; i < h; i++) memcpy((PIX*)r.y + (size_t)i * r.stride_y, &tmp[(size_t)i * w], w * sizeof(PIX));
    const PIX* cu = &tmp[(size_t)w * h]; const PIX* cv = cu + (size_t)(w / 2) * (h / 2);
    for (int i = 0; i < h / 2; i++) {
      memcpy((PIX*)r.u + (size_t)i * r.stride_c, cu + (size_t)i * (w / 2), (w / 2) * sizeof(PIX));
      memcpy((PIX*)r.v + (size_t)i * r.stride_c, cv + (size_t)i * (w / 2), (w / 2) * sizeof(PIX));
    }
  }
  // deblock_data[] as copy_deblock_data leaves it (enc/encode_block.c:1568-1613): the device keeps it as 16-byte DbCells
  if (ei->deblock_data) {
    std::vector<DbCell> cells(eng.num_cells());
    eng.download_cells(0, cells.data());
    for (size_t i = 0; i < cells.size(); i++) {
      const DdFields c = dd_fields(cells[i]);
      thor_deblock_data& d = ei->deblock_data[i];
      d.mode = c.mode; d.cbp_y = c.cbp_y; d.cbp_u = c.cbp_u; d.cbp_v = c.cbp_v;
      d.size = (uint8_t)c.size; d.tb_split = (uint8_t)c.tb_split; d.pb_part = c.pb_part;
      d.inter_pred.mv0.x = (int16_t)c.mv0x; d.inter_pred.mv0.y = (int16_t)c.mv0y;
      d.inter_pred.mv1.x = (int16_t)c.mv1x; d.inter_pred.mv1.y = (int16_t)c.mv1y;
      d.inter_pred.ref_idx0 = (uint32_t)c.ref_idx0; d.inter_pred.ref_idx1 = (uint32_t)c.ref_idx1; d.inter_pred.bipred_flag = (uint32_t)c.bipred_flag;
    }
  }
  // sliding window of the caller's reference pointers + padded copy (enc/encode_frame.c:826-835)
  {
    thor_yuv_frame* last = ei->ref[THOR_MAX_REF_FRAMES - 1];
    memmove(ei->ref + 1, ei->ref, sizeof(thor_yuv_frame*) * (THOR_MAX_REF_FRAMES - 1));
    ei->ref[0] = last;
    thor_yuv_frame& d = *ei->ref[0];
    const DevFrame<PIX>& g = eng.st[0].ring[0];
    d.frame_num = ei->rec->frame_num;
    const int ph = d.pad_ver_y, pw = d.pad_hor_y, pch = d.pad_ver_c, pcw = d.pad_hor_c;
    auto pull = [&](PIX* hp, int hs, const PIX* dp, int ds, int w, int h, int padw, int padh) {
      std::vector<PIX> buf((size_t)(h + 2 * padh) * ds);
      backend::d2h(buf.data(), dp - (size_t)padh * ds - padw, (buf.size() - (size_t)(ds - (w + 2 * padw))) * sizeof(PIX));
      for (int i = -padh; i < h + padh; i++)
        memcpy(hp + (ptrdiff_t)i * hs - padw, &buf[(size_t)(i + padh) * ds], (w + 2 * padw) * sizeof(PIX));
    };
    pull((PIX*)d.y, d.stride_y, g.p.y, g.p.sy, ei->width, ei->height, pw < kPadY ? pw : kPadY, ph < kPadY ? ph : kPadY);
    pull((PIX*)d.u, d.stride_c, g.p.u, g.p.sc, ei->width / 2, ei->height / 2, pcw < kPadY / 2 ? pcw : kPadY / 2, pch < kPadY / 2 ? pch : kPadY / 2);
    pull((PIX*)d.v, d.stride_c, g.p.v, g.p.sc, ei->width / 2, ei->height / 2, pcw < kPadY / 2 ? pcw : kPadY / 2, pch < kPadY / 2 ? pch : kPadY / 2);
  }
  ei->cdef_damping = 5;
}

extern "C" void encode_frame_lbd(struct thor_encoder_info* ei) { encode_frame_impl<uint8_t>(ei); }
extern "C" void encode_frame_hbd(struct thor_encoder_info* ei) { encode_frame_impl<uint16_t>(ei); }
