// The sliver of the range-v3 interface that the reference ricepp codec uses, written over <ranges> from the
// C++ standard's description of these views ([range.all], [range.drop], and P2442 chunk / stride as adopted in
// C++23).  TEST INFRASTRUCTURE ONLY: on the include path of oracle/ref_build.py, nothing else includes it.
//
// Only random-access sized ranges are supported (the codec views a std::span), which lets every view be a
// (base begin iterator, index) pair: no past-the-end arithmetic, no caching.
#pragma once

#include <algorithm>
#include <cstddef>
#include <iterator>
#include <limits>  // (range-v3's headers bring it in, and the codec relies on that)
#include <ranges>
#include <type_traits>
#include <utility>

namespace ranges {

template <typename R>
concept viewable_range = std::ranges::viewable_range<R>;

template <typename R>
using range_value_t = std::ranges::range_value_t<R>;

template <typename R>
  requires std::ranges::bidirectional_range<R>
constexpr void reverse(R&& r) {
  std::ranges::reverse(std::forward<R>(r));
}

namespace shim {

template <typename V>
concept base_view = std::ranges::view<V> && std::ranges::random_access_range<V> && std::ranges::sized_range<V>;

// ---- stride: every n-th element, ceil(size / n) of them ([range.stride]) ----
template <base_view V>
class stride_view : public std::ranges::view_interface<stride_view<V>> {
  using base_iterator = std::ranges::iterator_t<V>;

 public:
  using difference_type = std::ranges::range_difference_t<V>;

  class iterator {
   public:
    using iterator_category = std::random_access_iterator_tag;
    using iterator_concept = std::random_access_iterator_tag;
    using value_type = std::ranges::range_value_t<V>;
    using difference_type = typename stride_view::difference_type;
    using reference = std::ranges::range_reference_t<V>;
    using pointer = void;

    iterator() = default;
    constexpr iterator(base_iterator first, difference_type n, difference_type i)
        : first_{first}, n_{n}, i_{i} {}

    constexpr reference operator*() const { return first_[i_ * n_]; }
    constexpr reference operator[](difference_type k) const { return first_[(i_ + k) * n_]; }
    constexpr iterator& operator++() { ++i_; return *this; }
    constexpr iterator operator++(int) { auto t = *this; ++i_; return t; }
    constexpr iterator& operator--() { --i_; return *this; }
    constexpr iterator operator--(int) { auto t = *this; --i_; return t; }
    constexpr iterator& operator+=(difference_type k) { i_ += k; return *this; }
    constexpr iterator& operator-=(difference_type k) { i_ -= k; return *this; }
    friend constexpr iterator operator+(iterator a, difference_type k) { return a += k; }
    friend constexpr iterator operator+(difference_type k, iterator a) { return a += k; }
    friend constexpr iterator operator-(iterator a, difference_type k) { return a -= k; }
    friend constexpr difference_type operator-(iterator const& a, iterator const& b) { return a.i_ - b.i_; }
    friend constexpr bool operator==(iterator const& a, iterator const& b) { return a.i_ == b.i_; }
    friend constexpr auto operator<=>(iterator const& a, iterator const& b) { return a.i_ <=> b.i_; }

   private:
    base_iterator first_{};
    difference_type n_{1};
    difference_type i_{0};
  };

  stride_view() = default;
  constexpr stride_view(V base, difference_type n) : base_{std::move(base)}, n_{n} {}

  constexpr iterator begin() const { return {std::ranges::begin(base_), n_, 0}; }
  constexpr iterator end() const { return {std::ranges::begin(base_), n_, count()}; }
  constexpr std::size_t size() const { return static_cast<std::size_t>(count()); }

 private:
  constexpr difference_type count() const {
    return (static_cast<difference_type>(std::ranges::size(base_)) + n_ - 1) / n_;
  }

  V base_{};
  difference_type n_{1};
};

// ---- chunk: consecutive subranges of n elements, the last one shorter ([range.chunk]) ----
template <base_view V>
class chunk_view : public std::ranges::view_interface<chunk_view<V>> {
  using base_iterator = std::ranges::iterator_t<V>;

 public:
  using difference_type = std::ranges::range_difference_t<V>;
  using chunk_type = std::ranges::subrange<base_iterator>;

  class iterator {
   public:
    using iterator_category = std::input_iterator_tag;
    using iterator_concept = std::forward_iterator_tag;
    using value_type = chunk_type;
    using difference_type = typename chunk_view::difference_type;
    using reference = chunk_type;
    using pointer = void;

    iterator() = default;
    constexpr iterator(base_iterator first, difference_type size, difference_type n, difference_type at)
        : first_{first}, size_{size}, n_{n}, at_{at} {}

    constexpr chunk_type operator*() const {
      return {first_ + at_, first_ + std::min(size_, at_ + n_)};
    }
    constexpr iterator& operator++() { at_ = std::min(size_, at_ + n_); return *this; }
    constexpr iterator operator++(int) { auto t = *this; ++*this; return t; }
    friend constexpr bool operator==(iterator const& a, iterator const& b) { return a.at_ == b.at_; }

   private:
    base_iterator first_{};
    difference_type size_{0};
    difference_type n_{1};
    difference_type at_{0};
  };

  chunk_view() = default;
  constexpr chunk_view(V base, difference_type n) : base_{std::move(base)}, n_{n} {}

  constexpr iterator begin() const { return {std::ranges::begin(base_), total(), n_, 0}; }
  constexpr iterator end() const { return {std::ranges::begin(base_), total(), n_, total()}; }
  constexpr std::size_t size() const { return static_cast<std::size_t>((total() + n_ - 1) / n_); }

 private:
  constexpr difference_type total() const { return static_cast<difference_type>(std::ranges::size(base_)); }

  V base_{};
  difference_type n_{1};
};

// ---- closures: `range | views::chunk(n)`, `| views::drop(n)`, `| views::stride(n)` ----
struct chunk_closure { std::ptrdiff_t n; };
struct drop_closure { std::ptrdiff_t n; };
struct stride_closure { std::ptrdiff_t n; };

template <std::ranges::viewable_range R>
constexpr auto operator|(R&& r, chunk_closure c) {
  using V = std::views::all_t<R>;
  return chunk_view<V>{std::views::all(std::forward<R>(r)), static_cast<std::ranges::range_difference_t<V>>(c.n)};
}

template <std::ranges::viewable_range R>
constexpr auto operator|(R&& r, stride_closure c) {
  using V = std::views::all_t<R>;
  return stride_view<V>{std::views::all(std::forward<R>(r)), static_cast<std::ranges::range_difference_t<V>>(c.n)};
}

// the first min(n, size) elements dropped ([range.drop])
template <std::ranges::viewable_range R>
  requires base_view<std::views::all_t<R>>
constexpr auto operator|(R&& r, drop_closure c) {
  auto v = std::views::all(std::forward<R>(r));
  auto const size = static_cast<std::ptrdiff_t>(std::ranges::size(v));
  auto first = std::ranges::begin(v);
  return std::ranges::subrange{first + std::min(c.n, size), first + size};
}

struct chunk_fn {
  constexpr chunk_closure operator()(std::size_t n) const { return {static_cast<std::ptrdiff_t>(n)}; }
};
struct drop_fn {
  constexpr drop_closure operator()(std::size_t n) const { return {static_cast<std::ptrdiff_t>(n)}; }
};
struct stride_fn {
  constexpr stride_closure operator()(std::size_t n) const { return {static_cast<std::ptrdiff_t>(n)}; }
};

} // namespace shim

namespace views {
inline constexpr auto all = std::views::all;
inline constexpr shim::chunk_fn chunk{};
inline constexpr shim::drop_fn drop{};
inline constexpr shim::stride_fn stride{};
} // namespace views

} // namespace ranges
