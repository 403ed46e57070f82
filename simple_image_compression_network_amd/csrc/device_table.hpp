// How the ragged objects (k_ragged*.hip) own what they hold on the device, and how they come to be: a table that frees itself, the
// item -> owner map every flat grid reads, the ONE create path and the workspace check every async entry makes.  Host code only.
// The device calls (hipMalloc, hipFree, hipMemcpy, hipSuccess, hipMemcpyHostToDevice) are HIP's under hipcc; a program without HIP
// declares them itself before it includes this file (tests/cpp/device_table_check.cpp stands in for the device that way).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include <new>
#include <utility>
#include <vector>

#include "../../include/sicn.h"

namespace sicn {

// One array in device memory, owned: move-only, freed by the destructor — also after an upload whose copy failed.
template <class T>
class DeviceTable {
public:
    DeviceTable() = default;
    DeviceTable(DeviceTable &&o) noexcept { swap(o); }
    DeviceTable &operator=(DeviceTable &&o) noexcept
    {
        swap(o);            // what this table held goes with `o`
        return *this;
    }
    DeviceTable(const DeviceTable &) = delete;
    DeviceTable &operator=(const DeviceTable &) = delete;
    ~DeviceTable()
    {
        if (p_) (void)hipFree(p_);
    }

    // false: the allocation or the copy failed (memory whose copy failed stays owned).  No elements: nothing is allocated and the
    // table is null.
    bool upload(const T *host, size_t count)
    {
        DeviceTable().swap(*this);
        if (!count) return true;
        if (hipMalloc((void **)&p_, count * sizeof(T)) != hipSuccess) {
            p_ = nullptr;
            return false;
        }
        n_ = count;
        return hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
    }
    bool upload(const std::vector<T> &host) { return upload(host.data(), host.size()); }

    const T *get() const { return p_; }
    T *mut() { return p_; }             // for a kernel that writes the table (the rows of a moving ROI's last placement)
    size_t size() const { return n_; }

private:
    void swap(DeviceTable &o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
    T *p_ = nullptr;
    size_t n_ = 0;
};

// The map of a flat grid: map[item] = the image, slot or entry the work item belongs to, so that ONE load resolves item -> owner.
class ItemMap {
public:
    // `count` further items of `owner`; returns the first of them
    uint32_t add(size_t count, uint32_t owner)
    {
        const uint32_t first = (uint32_t)map_.size();
        map_.insert(map_.end(), count, owner);
        return first;
    }
    size_t size() const { return map_.size(); }
    bool upload(DeviceTable<uint32_t> &table) const { return table.upload(map_); }   // an empty grid has no table

private:
    std::vector<uint32_t> map_;
};

// The create path of every ragged object: *out = a new T that build(T &) filled, or nullptr and build's code — SICN_EINVAL for a
// null `out`, SICN_ENOMEM where the host has no memory (here or, as std::bad_alloc, anywhere in build).  What build had uploaded
// before it failed goes with the object.
template <class T, class F>
int make_object(T **out, F build)
{
    if (!out) return SICN_EINVAL;
    *out = nullptr;
    T *obj = new (std::nothrow) T();
    if (!obj) return SICN_ENOMEM;
    int rc;
    try {
        rc = build(*obj);
    } catch (const std::bad_alloc &) { rc = SICN_ENOMEM; }
    if (rc) {
        delete obj;
        return rc;
    }
    *out = obj;
    return SICN_OK;
}

// The caller's workspace of an async entry: SICN_ENOSPC without one or below `need` bytes, SICN_EINVAL off a 16-byte boundary.
inline int workspace_rc(const void *workspace, size_t bytes, uint64_t need)
{
    if (!workspace || bytes < need) return SICN_ENOSPC;
    return (reinterpret_cast<uintptr_t>(workspace) & 15) ? SICN_EINVAL : SICN_OK;
}

}  // namespace sicn
