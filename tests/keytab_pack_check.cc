// The packer of the key-table kernels' auxiliary block (audiowmark_amd/csrc/host/keytab_stage.hh) without a device: a stand-alone program
// for the address and undefined-behaviour sanitizers (tests/test_keytab_pack_host.py builds and runs it).
//
// 1, 3 and 257 keys, with and without a payload's coded bytes, through both forms of the packer (keys 16 bytes apart; a callable), each
// into a heap block of exactly the size the packer returns: the S-box, the coded bytes and every key schedule are where the returned
// offsets say, the schedules equal Aes128::round_keys() computed here, and the arguments of a launch point into the block.
#include "keytab_stage.hh"
#include <cstdio>
#include <memory>
#include <vector>

using namespace awm;

struct Args                                   // the fields of awmk::KeyTableArgs (hip/kernels.hh)
{
  const unsigned char *round_keys, *sbox, *coded;
  unsigned char       *scratch;
  int                  scratch_slots;
  signed char         *tables;
  long long            n_keys;
};

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf ("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void
check (size_t n_keys, bool with_code, bool callable)
{
  std::vector<uint8_t> keys (16 * n_keys);
  for (size_t i = 0; i < keys.size(); i++)
    keys[i] = uint8_t (i * 197 + n_keys * 31 + (i >> 8));
  std::vector<unsigned char> coded (2 * KEYTAB_CODE_BITS);
  for (size_t i = 0; i < coded.size(); i++)
    coded[i] = (unsigned char) ((i * i + i / 7) & 1);
  const unsigned char *code = with_code ? coded.data() : nullptr;

  const KeytabAux want = keytab_aux_layout (n_keys, with_code);
  CHECK (want.coded == 256 && want.schedules == 256 + (with_code ? 2 * 858 : 0) && want.bytes == want.schedules + 176 * n_keys);
  std::unique_ptr<unsigned char[]> block (new unsigned char[want.bytes]);
  const uint8_t *k = keys.data();
  const KeytabAux lay = callable ? keytab_aux_pack (block.get(), n_keys, [k] (size_t i) { return k + 16 * i; }, code)
                                 : keytab_aux_pack (block.get(), n_keys, k, code);
  CHECK (lay.coded == want.coded && lay.schedules == want.schedules && lay.bytes == want.bytes);
  CHECK (!std::memcmp (block.get(), Aes128::sbox(), KEYTAB_SBOX_BYTES));
  if (with_code)
    CHECK (!std::memcmp (block.get() + lay.coded, coded.data(), coded.size()));
  for (size_t i = 0; i < n_keys; i++)
    {
      Aes128 aes;
      aes.set_key (k + 16 * i);
      CHECK (!std::memcmp (block.get() + lay.schedules + KEYTAB_SCHEDULE_BYTES * i, aes.round_keys(), KEYTAB_SCHEDULE_BYTES));
    }
  // a launch of the last keys of the block
  const size_t first = n_keys > 256 ? 256 : 0;
  unsigned char scratch[1];
  const Args a = keytab_args<Args> (block.get(), lay, first, n_keys - first, scratch, 256);
  CHECK (a.sbox == block.get() && a.coded == (with_code ? block.get() + 256 : nullptr));
  CHECK (a.round_keys == block.get() + lay.schedules + 176 * first && a.round_keys + 176 * a.n_keys == block.get() + lay.bytes);
  CHECK (a.scratch == scratch && a.scratch_slots == 256 && a.tables == nullptr && a.n_keys == (long long) (n_keys - first));
}

int
main()
{
  for (size_t n_keys : { 1, 3, 257 })
    for (int with_code = 0; with_code < 2; with_code++)
      for (int callable = 0; callable < 2; callable++)
        check (n_keys, with_code, callable);
  if (failures)
    std::printf ("keytab pack check: %d FAILED\n", failures);
  else
    std::printf ("keytab pack check: ok\n");
  return failures ? 1 : 0;
}
