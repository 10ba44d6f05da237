// What the host stages for the key-table kernels (K16, K16t, K16g: hip/keytab.hip), in one place.
//
// The auxiliary block of a run of keys, one upload:
//
//   [S-box 256][conv code of one payload, A then B: 2 x 858 bytes 0 / 1 -- only K16 reads it][key schedules: n x 176]
//
// keytab_aux_pack writes it, keytab_args points a launch of 256 keys or fewer into it.  The packer needs aes128.hh and the standard
// library only (tests/keytab_pack_check.cc runs it under the sanitizers without a device).
#pragma once
#include "aes128.hh"
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace awmk { struct KeyTableArgs; }                     // hip/kernels.hh

namespace awm {

constexpr size_t KEYTAB_SBOX_BYTES = 256, KEYTAB_SCHEDULE_BYTES = 176, KEYTAB_CODE_BITS = 858;   // (coded bits per block type)

/* offsets into a packed block (bytes): the coded bytes, the first key schedule, the end */
struct KeytabAux
{
  size_t coded, schedules, bytes;
};

constexpr KeytabAux
keytab_aux_layout (size_t n_keys, bool with_code)
{
  return { KEYTAB_SBOX_BYTES, KEYTAB_SBOX_BYTES + (with_code ? 2 * KEYTAB_CODE_BITS : 0),
           KEYTAB_SBOX_BYTES + (with_code ? 2 * KEYTAB_CODE_BITS : 0) + n_keys * KEYTAB_SCHEDULE_BYTES };
}

/* packs the block of n_keys keys into dst (keytab_aux_layout (n_keys, coded).bytes bytes); key_at (i) -> the 16 bytes of key i;
 * coded: 2 x 858 bytes, A then B, or nullptr: a block without them (K16t, K16g) */
template<class KeyAt> KeytabAux
keytab_aux_pack (unsigned char *dst, size_t n_keys, KeyAt key_at, const unsigned char *coded = nullptr)
{
  const KeytabAux lay = keytab_aux_layout (n_keys, coded != nullptr);
  std::memcpy (dst, Aes128::sbox(), KEYTAB_SBOX_BYTES);
  if (coded)
    std::memcpy (dst + lay.coded, coded, 2 * KEYTAB_CODE_BITS);
  for (size_t i = 0; i < n_keys; i++)
    {
      Aes128 aes;
      aes.set_key (key_at (i));
      std::memcpy (dst + lay.schedules + KEYTAB_SCHEDULE_BYTES * i, aes.round_keys(), KEYTAB_SCHEDULE_BYTES);
    }
  return lay;
}

/* the same for keys that lie 16 bytes apart */
inline KeytabAux
keytab_aux_pack (unsigned char *dst, size_t n_keys, const uint8_t *keys, const unsigned char *coded = nullptr)
{
  return keytab_aux_pack (dst, n_keys, [keys] (size_t i) { return keys + 16 * i; }, coded);
}

/* the arguments of one launch: keys first_key .. first_key + n_keys - 1 of the block packed with layout `lay` that lies at d_aux on
 * the device.  The outputs (KeyTableArgs::tables, KeyTemplateOut, ClipKeyTableOut) are the caller's.  (Args: awmk::KeyTableArgs, a
 * template parameter only so that this header does not need the HIP runtime's) */
template<class Args = awmk::KeyTableArgs> Args
keytab_args (const unsigned char *d_aux, const KeytabAux& lay, size_t first_key, size_t n_keys, unsigned char *scratch, size_t scratch_slots)
{
  Args ka {};
  ka.sbox = d_aux;
  ka.coded = lay.schedules != lay.coded ? d_aux + lay.coded : nullptr;
  ka.round_keys = d_aux + lay.schedules + KEYTAB_SCHEDULE_BYTES * first_key;
  ka.scratch = scratch;
  ka.scratch_slots = int (scratch_slots);
  ka.n_keys = (long long) n_keys;
  return ka;
}

} // namespace awm
