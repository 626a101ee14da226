// amt_pass.hip -- the host path the streaming passes around the acoustic loop share (amt_pass.h).
// Host code only: the kernels, their job structs and their grids are the passes' own.
#include "amt_internal.h"

int amt_pass_check_arrays(const char *who, int members, const AmtPassArray *arr, int narr)
{
    for (int k = 0; k < narr; ++k)
        if (!arr[k].p && !arr[k].optional) return amt_fail(AMT_ERR_INVALID_ARG, "%s: null array pointer", who);
    if (members < 1) return amt_fail(AMT_ERR_INVALID_ARG, "%s: members = %d: an ensemble has at least one member", who, members);
    return AMT_OK;
}

int amt_pass_check_box(const char *who, const amt_domain &s, int members, const AmtPassArray *arr, int narr, const AmtPassRules &rules,
                       bool *empty)
{
    *empty = false;
    if (s.ime < s.ims || s.jme < s.jms || s.kme < s.kms) return amt_fail(AMT_ERR_PRECONDITION, "%s: empty memory extents", who);
    const size_t idim = s.ime - s.ims + 1, kdim = s.kme - s.kms + 1, jdim = s.jme - s.jms + 1, wb = (size_t)s.dtype_bytes;
    const size_t bytes[4] = {0, kdim * wb, idim * jdim * (size_t)members * wb, idim * kdim * jdim * (size_t)members * wb};
    for (int k = 0; k < narr; ++k) {
        if (!arr[k].p) continue;
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(arr[k].p), pb = bytes[arr[k].rank];
        for (int m = k + 1; m < narr; ++m) {
            if (!arr[m].p || !(arr[k].output || arr[m].output)) continue;
            const uintptr_t r0 = reinterpret_cast<uintptr_t>(arr[m].p), rb = bytes[arr[m].rank];
            if (p0 < r0 + rb && r0 < p0 + pb)
                return amt_fail(AMT_ERR_INVALID_ARG, "%s: %s", who,
                                arr[k].output && arr[m].output ? rules.output_overlaps_output : rules.output_overlaps_input);
        }
    }
    if (s.kts != 1) return amt_fail(AMT_ERR_PRECONDITION, "%s: kts = %d, the library needs kts == 1", who, s.kts);
    if (s.kte != s.kde) return amt_fail(AMT_ERR_PRECONDITION, "%s: kte = %d is not kde = %d", who, s.kte, s.kde);
    if (s.kme < s.kte || s.kms > s.kts) return amt_fail(AMT_ERR_PRECONDITION, "%s: levels kts:kte = %d:%d are not inside memory kms:kme = %d:%d", who, s.kts, s.kte, s.kms, s.kme);
    if (s.ite < s.its || s.jte < s.jts || s.kte - s.kts + 1 < rules.min_levels) { *empty = true; return AMT_OK; }
    if (s.its < s.ims || s.ite > s.ime || s.jts < s.jms || s.jte > s.jme)
        return amt_fail(AMT_ERR_PRECONDITION, "%s: the tile %d:%d, %d:%d is not inside memory %d:%d, %d:%d", who,
                        s.its, s.ite, s.jts, s.jte, s.ims, s.ime, s.jms, s.jme);
    if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one launch covers at most 65535", who, members);
    if (rules.needs_mass_column) {
        int ni, nj;
        amt_pass_mass_lengths(s, &ni, &nj);
        if (ni < 1 || nj < 1) *empty = true;
    }
    return AMT_OK;
}

void amt_pass_mass_lengths(const amt_domain &d, int *ni, int *nj)
{
    *ni = (d.ite < d.ide - 1 ? d.ite : d.ide - 1) - d.its + 1;
    *nj = (d.jte < d.jde - 1 ? d.jte : d.jde - 1) - d.jts + 1;
}

unsigned amt_pass_blocks(long items)
{
    const long blocks = (items + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks);
}

int amt_pass_current_device(int *device)
{
    int ndev = 0;
    AMT_HIP(hipGetDeviceCount(&ndev));
    if (ndev < 1) return amt_fail(AMT_ERR_NO_DEVICE, "no HIP device visible");
    (void)hipGetDevice(device);
    return AMT_OK;
}

int amt_pass_setting_offer(const char *who, const AmtPassSetting &s, void *const *arr, int *given, bool *same)
{
    *given = 0;
    for (int k = 0; k < s.count; ++k) *given += arr[k] != nullptr;
    if (*given != 0 && *given != s.count)
        return amt_fail(AMT_ERR_INVALID_ARG, "%s: give all %s or none (the library then allocates them)", who, s.all_of_them);
    *same = *given == s.count && *s.owned && memcmp(arr, s.slot, s.count * sizeof(void *)) == 0;
    return AMT_OK;
}

int amt_pass_setting_take(const char *who, const amt_domain *d, int members, const AmtPassSetting &s, void *const *arr, int given,
                          bool same, const std::function<int(void *const *)> &check)
{
    void *mine[9] = {};
    if (given) {
        if (*s.owned && !same)
            for (int k = 0; k < s.count; ++k)
                for (int m = 0; m < s.count; ++m)
                    if (s.slot[k] == arr[m]) return amt_fail(AMT_ERR_INVALID_ARG, "%s: %s the library allocated, mixed with others", who, s.one_of_them);
        const int rc = check(arr);                                 // against the caller's arrays, nothing enqueued
        if (rc) return rc;
        memcpy(mine, arr, s.count * sizeof(void *));
    } else {
        if (members > 65535) return amt_fail(AMT_ERR_PRECONDITION, "%s: %d members: one launch covers at most 65535", who, members);
        if (d->kts != 1 || d->kte != d->kde || d->kme < d->kte || d->kms > d->kts || d->its < d->ims || d->ite > d->ime || d->jts < d->jms || d->jte > d->jme)
            return amt_fail(AMT_ERR_PRECONDITION, "%s: the handle's tile does not admit %s (kts == 1, kte == kde, tile inside memory)", who, s.pass);
    }
    DeviceScope scope(d->device);                                  // behind every refusal but a failed allocation
    if (!given)
        for (int k = 0; k < s.count; ++k)
            if (hipMalloc(&mine[k], s.bytes[k]) != hipSuccess) {
                (void)hipGetLastError();
                for (int m = 0; m < k; ++m) (void)hipFree(mine[m]);
                return amt_fail(AMT_ERR_ALLOC, "%s: no room for %s of %zu bytes", who, s.room, s.bytes[k]);
            }
    if (same) return AMT_OK;
    amt_pass_setting_release(s);
    memcpy(s.slot, mine, s.count * sizeof(void *));
    *s.owned = !given;
    return AMT_OK;
}

void amt_pass_setting_release(const AmtPassSetting &s)
{
    for (int k = 0; k < s.count; ++k) {
        if (s.slot[k] && *s.owned) (void)hipFree(s.slot[k]);
        s.slot[k] = nullptr;
    }
    *s.owned = false;
}

amt_domain amt_pass_domain(int dtype_bytes, void *hip_stream, AMT_BOUNDS_SIG)
{
    amt_domain d{dtype_bytes, 0, 0, 0, ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, kts, kte};
    d.stream = static_cast<hipStream_t>(hip_stream);
    return d;
}
