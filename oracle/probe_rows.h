// Array form of the function-level probes, with the row layouts and function numbers of vk_raytrace_amd/csrc/pt_probe.h, so that a test sends
// a few thousand states through one call.  Included inside the extern "C" block of pt_oracle.cpp (PROBE_FN(x) = orc_##x) and of
// ref_glue/ref_comp.cpp (PROBE_FN(x) = ref_##x) after the per-state probes it loops over; vec3, reflect, refract, PROBE_MIX and PROBE_SMOOTHSTEP are
// whatever the including file has in scope (glsl_math.h there, ref_glue/glsl_compat.h here): functions 9..12 and 14..21 are that side's GLSL built-ins
// (PROBE_MUL_* / PROBE_MAT3_MUL: the matrix products as that side writes them), 13 its Environment_sample (PROBE_FN(env_sample), defined by the includer).
static void PROBE_FN(shading_probe_row)(int fn, const float* in, float* out)
{
  const float *m = in, *N = in + 22, *T = in + 25, *B = in + 28, *V = in + 33, *L = in + 36;
  switch(fn)
  {
    case 0: case 1: PROBE_FN(bsdf_eval)(fn, m, N, T, B, in[31], in[32] != 0.0f, V, L, out, out + 3); break;
    case 2: case 3:
    {
      uint32_t seed;
      std::memcpy(&seed, in + 39, 4);
      PROBE_FN(bsdf_sample)(fn - 2, m, N, T, B, in[31], in[32] != 0.0f, V, &seed, out, out + 3, out + 6);
      std::memcpy(out + 7, &seed, 4);
      break;
    }
    case 4:
    {
      pt_SunAndSky ss;
      std::memcpy(&ss, in, sizeof(ss));
      PROBE_FN(sun_and_sky)(&ss, in + sizeof(ss) / 4, out);
      break;
    }
    case 5: PROBE_FN(spherical_uv)(in, out); break;
    case 6: PROBE_FN(coordinate_system)(in, out, out + 3); break;
    case 7: out[0] = PROBE_FN(range_attenuation)(in[0], in[1]); break;
    case 8: out[0] = PROBE_FN(spot_attenuation)(in, in + 3, in[6], in[7]); break;
    case 9: case 10: case 11:
    {
      const vec3 a(in[0], in[1], in[2]), b(in[3], in[4], in[5]);
      const vec3 r = fn == 9 ? reflect(a, b) : fn == 10 ? refract(a, b, in[6]) : PROBE_MIX(a, b, in[6]);
      out[0] = r.x; out[1] = r.y; out[2] = r.z;
      break;
    }
    case 12: out[0] = PROBE_SMOOTHSTEP(in[0], in[1], in[2]); break;
    case 13: PROBE_FN(env_sample)(in, out, nullptr); break;  // Environment_sample: xi[3] width height pad[3] EnvAccel[width * height] -> to_light[3] pdf
    case 14: case 15:
    {
      const vec3 a(in[0], in[1], in[2]), b(in[3], in[4], in[5]);
      const vec3 r = fn == 14 ? cross(a, b) : normalize(a);
      out[0] = r.x; out[1] = r.y; out[2] = r.z;
      break;
    }
    case 16: case 17:  // mat4 * vec4, vec4 * mat4: m[16] column-major, v[4]
    {
      mat4 m;
      for(int k = 0; k < 4; ++k)
        m.c[k] = vec4(in[4 * k], in[4 * k + 1], in[4 * k + 2], in[4 * k + 3]);
      const vec4 v(in[16], in[17], in[18], in[19]);
      const vec4 r = fn == 16 ? m * v : v * m;
      out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
      break;
    }
    case 18: case 19: case 20:  // M * vec4(p, 1), vec3(p * M), mat4(M) * vec4(p, 0): m[12] = the 4 columns of a mat4x3, p[3]
    {
      mat4x3 m;
      for(int k = 0; k < 4; ++k)
        m.c[k] = vec3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
      const vec3 p(in[12], in[13], in[14]);
      const vec3 r = fn == 18 ? PROBE_MUL_POINT(m, p) : fn == 19 ? PROBE_MUL_ROWVEC(p, m) : PROBE_MUL_DIR(m, p);
      out[0] = r.x; out[1] = r.y; out[2] = r.z;
      break;
    }
    case 22: PROBE_FN(sun_disk_sample)(in, out); break;  // EnvSample under Sun & Sky (env_sampling.glsl:111-125): pt_SunAndSky[24] seed -> lightDir[3] pdf seed
    case 21:
    {
      const vec3 r = PROBE_MAT3_MUL(vec3(in[0], in[1], in[2]), vec3(in[3], in[4], in[5]), vec3(in[6], in[7], in[8]), vec3(in[9], in[10], in[11]));
      out[0] = r.x; out[1] = r.y; out[2] = r.z;
      break;
    }
    default: break;
  }
}
int PROBE_FN(shading_probe)(int fn, uint64_t n, const float* in, int in_stride, float* out, int out_stride)
{
  if(fn < 0 || fn > 22)
    return -1;
  for(uint64_t i = 0; i < n; ++i)
    PROBE_FN(shading_probe_row)(fn, in + i * (uint64_t)in_stride, out + i * (uint64_t)out_stride);
  return 0;
}

// The scalar built-ins one at a time: rows of three words (a, b, c) -> one word.  fn: 0 step(a, b)  1 clamp(a, b, c)  2 sign(a)  3 fract(a)  4 mod(a, b)
// 5 atan(a, b)  6 roundEven(a).  Returns -1 for a function the including side has no definition of (PROBE_HAS_SCALAR_BUILTINS: glsl_compat.h defines all
// of them for the reference's shaders; glsl_math.h only step and clamp, the oracle's restatement has no other call site).
int PROBE_FN(glsl_builtin)(int fn, uint64_t n, const float* in, int in_stride, float* out, int out_stride)
{
#ifdef PROBE_HAS_SCALAR_BUILTINS
  if(fn < 0 || fn > 6)
    return -1;
#else
  if(fn < 0 || fn > 1)
    return -1;
#endif
  for(uint64_t i = 0; i < n; ++i)
  {
    const float a = in[i * (uint64_t)in_stride], b = in[i * (uint64_t)in_stride + 1], c = in[i * (uint64_t)in_stride + 2];
    float&      r = out[i * (uint64_t)out_stride];
    switch(fn)
    {
      case 0: r = PROBE_STEP(a, b); break;
      case 1: r = PROBE_CLAMP(a, b, c); break;
#ifdef PROBE_HAS_SCALAR_BUILTINS
      case 2: r = sign(a); break;
      case 3: r = fract(a); break;
      case 4: r = mod(a, b); break;
      case 5: r = atan(a, b); break;
      case 6: r = roundEven(a); break;
#endif
      default: break;
    }
  }
  return 0;
}
