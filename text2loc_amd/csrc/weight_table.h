// What every eval-mode weight loader does on the host before it touches the device, as plain host code (tests/weight_table_check.cpp
// walks it): the name -> tensor table of a caller's descriptor list with ONE error text per kind of mistake, and the host image of the
// ONE device blob a model part's packed weights live in. A loader stages everything through these two, returns at the first error
// having touched neither the context nor the device, and only then allocates, copies once and publishes. No HIP in here.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "t2l.h"

namespace t2l {

// The tensors of a descriptor list by name, optionally only those under a name prefix. A list with a null name, null data or
// numel <= 0 is refused as a whole; of two tensors of one name the later one counts. The table keeps the FIRST error it met
// (error()); every lookup after it still answers, so a loader may check ok() once per group of lookups.
class WeightTable {
 public:
  WeightTable(const char* who, const t2l_weight_desc* w, int n, const char* prefix = nullptr) : who_(who) {
    const size_t np = prefix ? strlen(prefix) : 0;
    for (int i = 0; i < n; ++i) {
      if (!w[i].name || !w[i].data || w[i].numel <= 0) {
        refuse(std::string("tensor ") + std::to_string(i) + (w[i].name ? std::string(" ('") + w[i].name + "')" : std::string()) +
               " has a null name, null data or numel <= 0");
        return;
      }
      if (!np || !strncmp(w[i].name, prefix, np)) map_[w[i].name] = &w[i];
    }
  }
  bool ok() const { return err_.empty(); }
  const std::string& error() const { return err_; }
  bool empty() const { return map_.empty(); }
  // an optional tensor: null when the list has none of that name
  const t2l_weight_desc* find(const std::string& name) const {
    auto it = map_.find(name);
    return it == map_.end() ? nullptr : it->second;
  }
  // a required tensor of `numel` elements (0: of any size): its data, or null with the error recorded
  const float* need(const std::string& name, int64_t numel) {
    const t2l_weight_desc* d = find(name);
    if (!d) return refuse("missing tensor '" + name + "'");
    if (numel && d->numel != numel) return wrong_size(name, std::to_string(numel));
    return d->data;
  }
  // a required table of `width`-element rows, however many: its data and the row count
  const float* need_rows(const std::string& name, int64_t width, int64_t* rows) {
    const float* t = need(name, 0);
    if (t && find(name)->numel % width) return wrong_size(name, "a multiple of " + std::to_string(width));
    if (t) *rows = find(name)->numel / width;
    return t;
  }
  // ... whose size is not what `needs` says
  const float* wrong_size(const std::string& name, const std::string& needs) {
    const t2l_weight_desc* d = find(name);
    return refuse("wrong size for '" + name + "' (has " + std::to_string(d ? d->numel : 0) + " elements, needs " + needs + ")");
  }
  // any other refusal in the entry point's name; always returns null
  const float* refuse(const std::string& what) {
    if (err_.empty()) err_ = who_ + ": " + what;
    return nullptr;
  }

 private:
  std::string who_, err_;
  std::unordered_map<std::string, const t2l_weight_desc*> map_;
};

// The host image of one device blob. add() copies an array in at the next multiple of `align` bytes (zero fill in between) and
// returns its byte offset; place() also remembers a pointer field that bind() aims at the array's copy once the blob has an address.
// 256 bytes is what one device allocation per array used to give every array; the cell encoder packs at 16.
class Staging {
 public:
  // `expect`: about how many bytes will be staged (address space only; growing past it costs a copy of what is staged so far)
  explicit Staging(size_t expect = 16u << 20) { h_.reserve(expect); }
  size_t add(const void* src, size_t bytes, size_t align = 256) {
    const size_t off = (h_.size() + align - 1) / align * align;
    h_.resize(off, 0);
    h_.insert(h_.end(), static_cast<const unsigned char*>(src), static_cast<const unsigned char*>(src) + bytes);
    return off;
  }
  template <typename T>
  size_t add(const std::vector<T>& v, size_t align = 256) {
    return add(v.data(), v.size() * sizeof(T), align);
  }
  template <typename P, typename T>
  void place(P** field, const std::vector<T>& v, size_t align = 256) {
    fix_.push_back({static_cast<const void*>(field), add(v, align)});
  }
  template <typename P>
  void place(P** field, const float* src, size_t n, size_t align = 256) {
    fix_.push_back({static_cast<const void*>(field), add(src, n * sizeof(float), align)});
  }
  const void* data() const { return h_.data(); }
  size_t bytes() const { return h_.size(); }
  void bind(char* base) const {
    for (const Fix& f : fix_) {
      char* p = base + f.off;
      memcpy(const_cast<void*>(f.field), &p, sizeof(p));
    }
  }

 private:
  struct Fix {
    const void* field;  // a pointer-typed member of the weights struct being built
    size_t off;
  };
  std::vector<unsigned char> h_;
  std::vector<Fix> fix_;
};

}  // namespace t2l
