/* sampler_surface_check.c - TEST-ONLY: the oracle's per-call exports for the sampler and the surface stage, compiled together with
 * oracle/zo_oracle.c under the address, undefined-behaviour and float-cast sanitizers and run over the tables and image sets that
 * tests/test_device_function_tables.py writes into a directory.  Over the whole table, non-finite operands included, the oracle must
 * index no texel outside its chain and perform no undefined cast: a clean exit says so.  Prints one line per job with a 64-bit FNV-1a of
 * the result words, which the test compares with the library's.
 *
 * jobs.bin: u32 jobs, then per job
 *   kind 0: u32 0, u32 function (the order of PLAIN below), u32 cases, the table
 *   kind 1: u32 1, seven slots { u32 present, [u32 w, u32 h, u32 as_image, w * h * 4 bytes] }, u32 slot (7: all seven, the material form), u32 srgb,
 *           u32 cases, the table (6 words per case) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/zo_oracle.h"

typedef void (*batch_fn)(const uint32_t*, uint32_t*, uint32_t);
static const struct { const char* name; batch_fn f; uint32_t in, out; } PLAIN[] = {
    { "tex_footprint", zo_kat_tex_footprint_batch, 7, 4 }, { "bary_screen", zo_kat_bary_screen_batch, 11, 3 },
    { "bary_homog", zo_kat_bary_homog_batch, 16, 3 },      { "interp", zo_kat_interp_batch, 12, 4 },
    { "compute_normal", zo_kat_compute_normal_batch, 16, 3 }, { "model_point", zo_kat_model_point_batch, 20, 3 },
};

static FILE* in;
static uint32_t get32(void)
{
    uint32_t v;
    if (fread(&v, 4, 1, in) != 1) { fprintf(stderr, "jobs.bin is cut\n"); exit(2); }
    return v;
}
/* a heap block of exactly n bytes: one byte past it is out of bounds to the sanitizer */
static void* get_block(size_t n)
{
    void* p = malloc(n ? n : 1);
    if (!p || (n && fread(p, 1, n, in) != n)) { fprintf(stderr, "jobs.bin is cut\n"); exit(2); }
    return p;
}
static uint64_t fnv1a(const void* p, size_t n)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 0x100000001B3ull;
    return h;
}

int main(int argc, char** argv)
{
    if (argc != 2 || !(in = fopen(argv[1], "rb"))) { fprintf(stderr, "usage: sampler_surface_check jobs.bin\n"); return 2; }
    zo_ctx* c = zo_create(8, 8, 8);
    const uint32_t jobs = get32();
    for (uint32_t j = 0; j < jobs; ++j) {
        const uint32_t kind = get32();
        uint32_t n, wi, wo;
        uint32_t *table, *out;
        if (kind == 0) {
            const uint32_t fn = get32();
            if (fn >= sizeof PLAIN / sizeof PLAIN[0]) return 2;
            n = get32(); wi = PLAIN[fn].in; wo = PLAIN[fn].out;
            table = (uint32_t*)get_block((size_t)n * wi * 4); out = (uint32_t*)calloc((size_t)n * wo, 4);
            PLAIN[fn].f(table, out, n);
            printf("%u %s %u %016llx\n", j, PLAIN[fn].name, n, (unsigned long long)fnv1a(out, (size_t)n * wo * 4));
        } else {
            for (int s = 0; s < 7; ++s) {
                if (!get32()) { zo_kat_set_image(c, s, NULL, 0, 0, 0, 0); continue; }
                const uint32_t w = get32(), h = get32(), as_image = get32();
                uint8_t* px = (uint8_t*)get_block((size_t)w * h * 4);
                if (zo_kat_set_image(c, s, px, w, h, s == 0, (int)as_image) < 1) return 2;
                free(px);
            }
            const uint32_t slot = get32(), srgb = get32();
            n = get32(); wi = 6; wo = slot == 7 ? 28 : 4;
            table = (uint32_t*)get_block((size_t)n * wi * 4); out = (uint32_t*)calloc((size_t)n * wo, 4);
            if (slot == 7) zo_kat_tex_material_batch(c, table, out, n);
            else zo_kat_tex_image_batch(c, (int)slot, (int)srgb, table, out, n);
            printf("%u %s %u %016llx\n", j, slot == 7 ? "tex_material" : "tex_image", n, (unsigned long long)fnv1a(out, (size_t)n * wo * 4));
        }
        free(table); free(out);
    }
    zo_destroy(c);
    fclose(in);
    return 0;
}
